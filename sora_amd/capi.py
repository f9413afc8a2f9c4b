"""ctypes binding of the C ABI in include/sora_hip.h (libsora_hip.so).

This is plumbing only: device memory comes from torch (or sora_hip_malloc), all compute is the HIP library.
The wrapper mirrors the reference harness: `Rx.process(...)` = RxThread over a batch of captures,
`Rx.results()` = the frames TBB11aFrameSink reported.  Nothing here falls back to a CPU implementation:
if the library or a GPU is missing, calls raise.
"""
import collections
import ctypes
import os

import numpy as np

from . import build as _build

SORA_OK = 0
E_FRAME_OK = 0x1
TRELLIS_WINDOWED = 1          # sora_rx_set_trellis: the window-parallel trellis (include/sora_hip.h SORA_TRELLIS_WINDOWED)
E_PLCP_HEADER_FAIL = 0x80000005
E_CRC32_FAIL = 0x80000006
E_SFD_FAIL = 0x80000004
E_CS_TIMEOUT = 0x80000007
E_SFD_TIMEOUT = 0x80000008
E_SYNC_TIMEOUT = 0x80000009
ERR_NO_DEVICE = -5
ERR_CAPACITY = -6


class SoraError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("sora_hip error %d (0x%08X): %s" % (code, code & 0xFFFFFFFF, msg))
        self.code = code


class RxCfg(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", ctypes.c_int32), ("sample_rate_mhz", ctypes.c_uint32),
                ("max_captures", ctypes.c_uint32), ("max_total_samples", ctypes.c_uint64),
                ("max_frames_per_capture", ctypes.c_uint32), ("cca_pwr_threshold", ctypes.c_uint32)]


class CaptureDesc(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("nsamples", ctypes.c_uint32), ("capture_id", ctypes.c_uint32)]


class FrameResult(ctypes.Structure):
    _fields_ = [("capture_id", ctypes.c_uint32), ("start_sample", ctypes.c_uint32), ("end_sample", ctypes.c_uint32),
                ("error_code", ctypes.c_uint32), ("rate_kbps", ctypes.c_uint32), ("length", ctypes.c_uint16),
                ("nsym", ctypes.c_uint16), ("crc32", ctypes.c_uint32), ("cfo_est", ctypes.c_int16),
                ("flags", ctypes.c_uint16), ("mpdu_offset", ctypes.c_uint32)]


class Ht40Frame(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("n_bpsc", ctypes.c_uint32), ("code_rate", ctypes.c_uint32), ("length", ctypes.c_uint32 * 2),
                ("cfo", ctypes.c_int32), ("noise_var", ctypes.c_float), ("frame_id", ctypes.c_uint32)]


class Ht40Found(ctypes.Structure):                      # sora_ht40_found: one record of the 40 MHz HT front end (sora_ht40_found_of)
    _fields_ = [("a20", ctypes.c_uint32), ("mcs", ctypes.c_uint32), ("ht_len", ctypes.c_uint32), ("nsym", ctypes.c_uint32), ("cfo", ctypes.c_int32),
                ("noise_var", ctypes.c_float), ("end_sample", ctypes.c_uint32), ("error_code", ctypes.c_uint32)]


EXPORTS = ["sora_hip_abi_version", "sora_hip_last_error", "sora_hip_device_count", "sora_hip_malloc", "sora_hip_free",
           "sora_hip_memcpy_h2d", "sora_hip_memcpy_d2h", "sora_hip_memcpy_d2d", "sora_hip_stream_synchronize", "sora_rx_create", "sora_rx_destroy", "sora_rx_reset",
           "sora_rx_flush", "sora_rx_stream", "sora_rx_process_dev", "sora_rx_process_dump", "sora_rx_set_stream_mode", "sora_rx_stream_consumed",
           "sora_rx_stream_record_of", "sora_rx_process", "sora_rx_results",
           "sora_rx_results_dev", "sora_rx_ticket", "sora_rx_wait", "sora_rx_wait_any", "sora_rx_results_of", "sora_rx_results_dev_of", "sora_rx_stream_of",
           "sora_rx_mpdu_bytes", "sora_rx_deliver_async", "sora_hip_host_alloc", "sora_hip_host_free", "sora_rx_set_profiling", "sora_rx_kernel_times", "sora_rx_kernel_name",
                      "sora_rx_set_depth", "sora_rx_set_fused", "sora_rx_set_trellis", "sora_rx_trellis", "sora_rx_window_stats", "sora_rx_set_front", "sora_rx_front",
                      "sora_rx_call_front", "sora_rx_set_ordered", "sora_hip_set_share_window_us", "sora_rx_set_pipe_wait_us", "sora_rx_pipe_stats", "sora_rx_bind_mpdu",
                      "sora_hip_table_count", "sora_hip_table_name", "sora_hip_table_pin", "sora_hip_table_digest", "sora_hip_table_read", "sora_rx_set_graph",
                      "sora_rx_kernel_name_fused", "sora_hip_fft64", "sora_hip_fft128", "sora_hip_lts11a", "sora_hip_symfront11a", "sora_hip_pilot_track11a", "sora_hip_pilot11a",
                      "sora_hip_freq_comp11a", "sora_hip_equalize11a", "sora_hip_phase_comp11a", "sora_hip_demap11a", "sora_hip_deinterleave11a", "sora_hip_viterbi11a",
                      "sora_hip_viterbi11a_ws", "sora_hip_viterbi11a_workspace_bytes", "sora_hip_viterbi11n_ws", "sora_hip_viterbi11n_workspace_bytes",
                      "sora_hip_viterbi_window_stats", "sora_hip_viterbi56_11n",
           "sora_hip_ingest", "sora_hip_ingest_count", "sora_hip_tx11a", "sora_hip_tx11a_samples", "sora_hip_tx11a44", "sora_hip_tx11a44_samples",
           "sora_hip_scramble11a", "sora_hip_conv_encode11a", "sora_hip_interleave11a", "sora_hip_map11a", "sora_hip_add_pilot11a", "sora_hip_add_pilot11a_from",
           "sora_hip_ifftx11a", "sora_hip_upsample40to44", "sora_hip_pack16to8", "sora_hip_preamble11a",
           "sora_hip_stream_parse11n", "sora_hip_interleave11n", "sora_hip_map11n", "sora_hip_sig_map11n", "sora_hip_add_pilot11n", "sora_hip_ifft_only11n",
           "sora_hip_csd11n", "sora_hip_add_gi11n", "sora_hip_preamble11n",
           "sora_hip_dc_remove11b", "sora_hip_energy_detect11b", "sora_hip_symtiming11b", "sora_hip_barker_sync11b", "sora_hip_despread11b", "sora_hip_sfd_sync11b",
           "sora_hip_dbpsk_demap11b", "sora_hip_dqpsk_demap11b", "sora_hip_cck5p5_decode11b", "sora_hip_cck11_decode11b", "sora_hip_desc741_11b", "sora_hip_plcp_parse11b",
           "sora_hip_frame_sink11b",
           "sora_hip_tx11n", "sora_hip_tx11n_samples", "sora_hip_tx_ht40", "sora_hip_tx_ht40_samples", "sora_hip_tx11b", "sora_hip_tx11b_samples", "sora_hip_tx11b_pre", "sora_hip_tx11b_pre_samples",
           "sora_hip_ppdu11b", "sora_hip_sc741_11b", "sora_hip_dbpsk_spread11b", "sora_hip_dqpsk_spread11b", "sora_hip_cck5_encode11b", "sora_hip_cck11_encode11b",
           "sora_hip_pulse_shape11b",
           "sora_hip_tx_ht40_joint", "sora_hip_tx_ht40_joint_samples",
           "sora_hip_tx_ht40_gi", "sora_hip_tx_ht40_gi_samples", "sora_hip_tx_ht40_joint_gi", "sora_hip_tx_ht40_joint_gi_samples",
           "sora_hip_tx_ht40_mcs", "sora_hip_tx_ht40_mcs_samples", "sora_hip_tx_ht40_joint_mcs", "sora_hip_tx_ht40_joint_mcs_samples",
           "sora_hip_stream_parse_ht40", "sora_hip_interleave_ht40", "sora_hip_interleave_ht40_stream", "sora_hip_map_ht40", "sora_hip_sig_map_ht40",
           "sora_hip_add_pilot_ht40", "sora_hip_ifft_ht40", "sora_hip_add_gi_ht40", "sora_hip_preamble_ht40",
           "sora_hip_demap11n", "sora_hip_deinterleave11n", "sora_hip_mimo_est11n", "sora_hip_mimo_comp11n", "sora_hip_cfo_est11n", "sora_hip_freq_comp11n",
                      "sora_hip_pilot_track11n", "sora_hip_siso_est11n", "sora_hip_siso_comp11n", "sora_hip_sig_demap11n", "sora_hip_sig_decode11n",
           "sora_hip_cca11n", "sora_hip_data_symbol11n", "sora_hip_stream_join11n", "sora_hip_desc11a", "sora_hip_frame_sink11a",
           "sora_hip_dc_remove11a", "sora_hip_dc_estimate11a", "sora_hip_cca11a", "sora_hip_carrier_sense11a", "sora_hip_data_symbol11a", "sora_hip_viterbi_sig11a",
           "sora_hip_plcp_parse11a",
           "sora_hip_data_symbol_ht40", "sora_hip_mimo_est_ht40", "sora_hip_mimo_comp_ht40", "sora_hip_pilot_track_ht40", "sora_hip_demap_ht40", "sora_hip_deinterleave_ht40",
           "sora_hip_stream_join_ht40", "sora_hip_downsample_ht40", "sora_hip_noise_var_ht40", "sora_rx11b_create",
                      "sora_rx11b_destroy", "sora_rx11b_stream", "sora_rx11b_synchronize", "sora_rx11b_process_dev", "sora_rx11b_process", "sora_rx11b_results", "sora_rx11b_ticket",
                      "sora_rx11b_calls_in_flight", "sora_rx11b_set_single_pass", "sora_rx11b_set_preamble", "sora_rx11b_wait", "sora_rx11b_wait_any", "sora_rx11b_stream_of", "sora_rx11b_results_of",
                      "sora_rx11b_deliver_async", "sora_rx11b_set_stream_mode", "sora_rx11b_stream_consumed", "sora_rx11n_deliver_async",
                      "sora_rx11n_set_stream_mode", "sora_rx11n_stream_consumed", "sora_ht40_deliver_async",
           "sora_rx11n_create", "sora_rx11n_destroy", "sora_rx11n_stream", "sora_rx11n_process_dev", "sora_rx11n_process", "sora_rx11n_results",
           "sora_rx11n_set_depth", "sora_rx11n_set_trellis", "sora_rx11n_trellis", "sora_rx11n_window_stats", "sora_rx11n_synchronize", "sora_rx11n_ticket", "sora_rx11n_wait",
                      "sora_rx11n_wait_any", "sora_rx11n_results_of", "sora_rx11n_set_mcs_max",
           "sora_ht40_symbols", "sora_ht40_create", "sora_ht40_destroy", "sora_ht40_stream", "sora_ht40_synchronize", "sora_ht40_set_trellis", "sora_ht40_process_dev",
                      "sora_ht40_process_captures_dev", "sora_ht40_results", "sora_ht40_ticket", "sora_ht40_calls_in_flight", "sora_ht40_wait", "sora_ht40_wait_any",
                      "sora_ht40_stream_of", "sora_ht40_results_of", "sora_ht40_soft_of", "sora_ht40_found_of", "sora_ht40_set_stream_mode", "sora_ht40_stream_consumed",
                      "sora_ht40_set_coding", "sora_ht40_symbols_joint", "sora_ht40_set_guard", "sora_ht40_set_mcs_max",
           "sora_shard_unique_id", "sora_shard_create", "sora_shard_destroy", "sora_shard_world", "sora_shard_partition", "sora_shard_gather_rows",
           "sora_shard_reduce_counters", "sora_shard_gather_results", "sora_shard_gather_results_mpdu"]

STREAM11B_STAGES = ("sora_hip_dbpsk_demap11b", "sora_hip_dqpsk_demap11b", "sora_hip_cck5p5_decode11b", "sora_hip_cck11_decode11b", "sora_hip_desc741_11b")

SPREAD11B_STAGES = ("sora_hip_dbpsk_spread11b", "sora_hip_dqpsk_spread11b", "sora_hip_cck5_encode11b", "sora_hip_cck11_encode11b")

_lib = None


def table_names():
    """the library's pinned look-up tables (include/sora_hip.h: sora_hip_table_*)"""
    L = load()
    return [L.sora_hip_table_name(i).decode() for i in range(L.sora_hip_table_count())]


def table_pin(name):
    r = load().sora_hip_table_pin(name.encode())
    return r.decode() if r else None


def table_digest(name):
    """sha256 of the table as this build on this host generates it (no device needed)"""
    buf = ctypes.create_string_buffer(65)
    _check(load().sora_hip_table_digest(name.encode(), buf))
    return buf.value.decode()


def table_read(name):
    """the device-resident table of the current device, as bytes"""
    L = load(); n = ctypes.c_size_t(0)
    _check(L.sora_hip_table_read(name.encode(), None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(n.value)
    _check(L.sora_hip_table_read(name.encode(), buf, n.value, ctypes.byref(n)))
    return buf.raw[:n.value]


def lib_path():
    return _build.LIB


def load(build_if_missing=True):
    """Load libsora_hip.so (building it with hipcc if absent).  Raises if it cannot be had."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm bundles its own libamdhip64 (same soname as /opt/rocm's).  Whichever copy is mapped first
    # serves the whole process, and torch only initialises against its own: import torch BEFORE dlopen-ing
    # libsora_hip.so so both share torch's runtime.  (A pure C host has no such concern.)
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    path = os.environ.get("SORA_HIP_LIB") or _build.LIB             # SORA_HIP_LIB: an experimental build of the same library (tools/ab_*.sh)
    if path == _build.LIB and build_if_missing and _build.needs_build():
        _build.build()
    if not os.path.exists(path):
        raise SoraError(-1, "libsora_hip.so is missing and could not be built; there is no CPU fallback")
    L = ctypes.CDLL(path)
    L.sora_hip_last_error.restype = ctypes.c_char_p
    L.sora_hip_malloc.restype = ctypes.c_void_p
    L.sora_hip_malloc.argtypes = [ctypes.c_size_t]
    L.sora_hip_free.argtypes = [ctypes.c_void_p]
    L.sora_hip_memcpy_h2d.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.sora_hip_memcpy_d2h.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.sora_rx_create.argtypes = [ctypes.POINTER(RxCfg), ctypes.POINTER(ctypes.c_void_p)]
    L.sora_rx_reset.argtypes = [ctypes.c_void_p]
    L.sora_rx_flush.argtypes = [ctypes.c_void_p]
    L.sora_rx_process_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(CaptureDesc), ctypes.c_size_t]
    L.sora_rx_process.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(CaptureDesc), ctypes.c_size_t]
    L.sora_rx_results.argtypes = [ctypes.c_void_p, ctypes.POINTER(FrameResult), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                  ctypes.c_void_p, ctypes.c_size_t]
    L.sora_rx_results_dev.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]
    L.sora_rx_results_dev_of.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]
    L.sora_rx_mpdu_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int]; L.sora_rx_mpdu_bytes.restype = ctypes.c_size_t
    L.sora_hip_host_alloc.argtypes = [ctypes.c_size_t]; L.sora_hip_host_alloc.restype = ctypes.c_void_p
    L.sora_hip_host_free.argtypes = [ctypes.c_void_p]; L.sora_hip_host_free.restype = None
    L.sora_rx_set_profiling.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx_kernel_times.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.sora_rx_kernel_name.argtypes = [ctypes.c_size_t]; L.sora_rx_kernel_name.restype = ctypes.c_char_p
    L.sora_rx_set_depth.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx_process_dump.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint, ctypes.POINTER(CaptureDesc), ctypes.c_size_t]
    L.sora_rx_set_fused.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx_set_trellis.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx_set_graph.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx_trellis.argtypes = [ctypes.c_void_p]
    L.sora_rx_window_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]
    L.sora_rx_set_front.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx_front.argtypes = [ctypes.c_void_p]
    L.sora_rx_call_front.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx_set_ordered.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_hip_set_share_window_us.argtypes = [ctypes.c_uint]; L.sora_hip_set_share_window_us.restype = ctypes.c_uint
    L.sora_rx_bind_mpdu.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.sora_rx_set_pipe_wait_us.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    L.sora_rx_pipe_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]
    L.sora_hip_table_count.argtypes = []
    L.sora_hip_table_name.argtypes = [ctypes.c_int]; L.sora_hip_table_name.restype = ctypes.c_char_p
    L.sora_hip_table_pin.argtypes = [ctypes.c_char_p]; L.sora_hip_table_pin.restype = ctypes.c_char_p
    L.sora_hip_table_digest.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    L.sora_hip_table_read.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.sora_rx11n_set_trellis.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx11n_trellis.argtypes = [ctypes.c_void_p]
    L.sora_rx11n_window_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]
    L.sora_ht40_set_trellis.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx_kernel_name_fused.argtypes = [ctypes.c_size_t]; L.sora_rx_kernel_name_fused.restype = ctypes.c_char_p
    L.sora_ht40_symbols.argtypes = [ctypes.c_uint32] * 4; L.sora_ht40_symbols.restype = ctypes.c_uint32
    L.sora_ht40_symbols_joint.argtypes = [ctypes.c_uint32] * 3; L.sora_ht40_symbols_joint.restype = ctypes.c_uint32
    L.sora_ht40_set_coding.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_ht40_set_guard.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_ht40_set_mcs_max.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_ht40_create.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]
    L.sora_ht40_process_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Ht40Frame), ctypes.c_size_t, ctypes.c_void_p]
    L.sora_ht40_results.argtypes = [ctypes.c_void_p, ctypes.POINTER(FrameResult), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p, ctypes.c_size_t]
    L.sora_shard_unique_id.argtypes = [ctypes.c_void_p]
    L.sora_shard_create.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.sora_shard_destroy.argtypes = [ctypes.c_void_p]; L.sora_shard_destroy.restype = None
    L.sora_shard_world.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.sora_shard_partition.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    L.sora_shard_partition.restype = None
    L.sora_shard_gather_rows.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.sora_shard_reduce_counters.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_shard_gather_results.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(FrameResult),
                                            ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_size_t)]
    L.sora_shard_gather_results_mpdu.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(FrameResult),
                                                 ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_size_t)]
    L.sora_hip_fft64.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_fft128.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_lts11a.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_symfront11a.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    for fn in ("sora_hip_freq_comp11a", "sora_hip_equalize11a", "sora_hip_phase_comp11a"):
        getattr(L, fn).argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_pilot_track11a.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_pilot11a.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_demap11a.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_deinterleave11a.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_viterbi11a.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_viterbi11a_workspace_bytes.argtypes = [ctypes.c_size_t, ctypes.c_size_t]; L.sora_hip_viterbi11a_workspace_bytes.restype = ctypes.c_size_t
    L.sora_hip_viterbi11a_ws.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    L.sora_hip_viterbi11n_workspace_bytes.argtypes = [ctypes.c_size_t, ctypes.c_size_t]; L.sora_hip_viterbi11n_workspace_bytes.restype = ctypes.c_size_t
    L.sora_hip_viterbi11n_ws.argtypes = L.sora_hip_viterbi11a_ws.argtypes
    L.sora_hip_viterbi_window_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_void_p]
    L.sora_hip_viterbi56_11n.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.c_void_p]
    L.sora_hip_stream_synchronize.argtypes = [ctypes.c_void_p]
    L.sora_hip_tx11a_samples.argtypes = [ctypes.c_uint32, ctypes.c_uint32]; L.sora_hip_tx11a_samples.restype = ctypes.c_size_t
    L.sora_hip_tx11a.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.sora_hip_tx11a44_samples.argtypes = [ctypes.c_uint32, ctypes.c_uint32]; L.sora_hip_tx11a44_samples.restype = ctypes.c_size_t
    L.sora_hip_tx11a44.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    # the 802.11a modulation graph's bricks as stages
    L.sora_hip_scramble11a.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_conv_encode11a.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_interleave11a.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_map11a.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_add_pilot11a.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    L.sora_hip_add_pilot11a_from.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    L.sora_hip_ifftx11a.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_upsample40to44.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_pack16to8.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_preamble11a.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    # the 802.11n modulation graphs' bricks as stages
    L.sora_hip_stream_parse11n.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_interleave11n.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_map11n.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_sig_map11n.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_add_pilot11n.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    L.sora_hip_ifft_only11n.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_csd11n.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_add_gi11n.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_preamble11n.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_stream_parse_ht40.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_interleave_ht40.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_interleave_ht40_stream.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_map_ht40.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_sig_map_ht40.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_add_pilot_ht40.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_ifft_ht40.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_add_gi_ht40.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_preamble_ht40.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    # the 802.11b receive graph's bricks as stages
    L.sora_hip_dc_remove11b.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    for fn in ("sora_hip_energy_detect11b", "sora_hip_barker_sync11b", "sora_hip_despread11b"):
        getattr(L, fn).argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_sfd_sync11b.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    L.sora_hip_symtiming11b.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    for fn in STREAM11B_STAGES:
        getattr(L, fn).argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_plcp_parse11b.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_frame_sink11b.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_tx11n_samples.argtypes = [ctypes.c_uint32, ctypes.c_uint32]; L.sora_hip_tx11n_samples.restype = ctypes.c_size_t
    L.sora_hip_tx11n.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t] + [ctypes.c_void_p] * 4
    L.sora_hip_tx_ht40_samples.argtypes = [ctypes.c_uint32, ctypes.c_uint32]; L.sora_hip_tx_ht40_samples.restype = ctypes.c_size_t
    L.sora_hip_tx_ht40.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t] + [ctypes.c_void_p] * 4
    L.sora_hip_tx_ht40_joint_samples.argtypes = [ctypes.c_uint32, ctypes.c_uint32]; L.sora_hip_tx_ht40_joint_samples.restype = ctypes.c_size_t
    L.sora_hip_tx_ht40_joint.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t] + [ctypes.c_void_p] * 4
    for fn in (L.sora_hip_tx_ht40_gi, L.sora_hip_tx_ht40_joint_gi):
        fn.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t] + [ctypes.c_void_p] * 4
    for fn in (L.sora_hip_tx_ht40_gi_samples, L.sora_hip_tx_ht40_joint_gi_samples):
        fn.argtypes = [ctypes.c_uint32] * 3; fn.restype = ctypes.c_size_t
    for fn in (L.sora_hip_tx_ht40_mcs, L.sora_hip_tx_ht40_joint_mcs):
        fn.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t] + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]
    for fn in (L.sora_hip_tx_ht40_mcs_samples, L.sora_hip_tx_ht40_joint_mcs_samples):
        fn.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_int]; fn.restype = ctypes.c_size_t
    L.sora_hip_tx11b_samples.argtypes = [ctypes.c_uint32, ctypes.c_uint32]; L.sora_hip_tx11b_samples.restype = ctypes.c_size_t
    L.sora_hip_tx11b.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t] + [ctypes.c_void_p] * 3
    L.sora_hip_tx11b_pre_samples.argtypes = [ctypes.c_uint32] * 3; L.sora_hip_tx11b_pre_samples.restype = ctypes.c_size_t
    L.sora_hip_tx11b_pre.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_size_t] + [ctypes.c_void_p] * 3
    # the 802.11b modulation graph's bricks as stages
    L.sora_hip_ppdu11b.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_size_t, ctypes.c_void_p]
    for fn in ("sora_hip_sc741_11b",) + SPREAD11B_STAGES:
        getattr(L, fn).argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_pulse_shape11b.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_ingest_count.argtypes = [ctypes.c_size_t, ctypes.c_uint]; L.sora_hip_ingest_count.restype = ctypes.c_size_t
    L.sora_hip_ingest.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t,
                                  ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
    L.sora_hip_demap11n.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_deinterleave11n.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_cfo_est11n.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_freq_comp11n.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_pilot_track11n.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_mimo_est11n.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_mimo_comp11n.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_siso_est11n.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_siso_comp11n.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_sig_demap11n.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_sig_decode11n.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_size_t, ctypes.c_void_p]
    # the bricks that complete the 802.11n receive graph
    L.sora_hip_cca11n.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p]
    L.sora_hip_data_symbol11n.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_stream_join11n.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_desc11a.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_frame_sink11a.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p]
    # the front end of the 802.11a receive graph
    L.sora_hip_dc_remove11a.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_dc_estimate11a.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_cca11a.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p]
    L.sora_hip_carrier_sense11a.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p]
    L.sora_hip_data_symbol11a.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_viterbi_sig11a.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_plcp_parse11a.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_size_t, ctypes.c_void_p]
    # the 40 MHz HT receiver's bricks as stages
    L.sora_hip_data_symbol_ht40.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_mimo_est_ht40.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_mimo_comp_ht40.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_pilot_track_ht40.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_demap_ht40.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_deinterleave_ht40.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_stream_join_ht40.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_downsample_ht40.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    L.sora_hip_noise_var_ht40.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p]
    L.sora_rx11n_create.argtypes = [ctypes.POINTER(RxCfg), ctypes.POINTER(ctypes.c_void_p)]
    L.sora_rx11n_process_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(CaptureDesc), ctypes.c_size_t]
    L.sora_rx11n_process.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(CaptureDesc), ctypes.c_size_t]
    L.sora_rx11n_set_depth.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx11n_set_mcs_max.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx11n_results.argtypes = [ctypes.c_void_p, ctypes.POINTER(FrameResult), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                     ctypes.c_void_p, ctypes.c_size_t]
    L.sora_rx11b_create.argtypes = [ctypes.POINTER(RxCfg), ctypes.POINTER(ctypes.c_void_p)]
    L.sora_rx11b_set_single_pass.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx11b_set_preamble.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sora_rx11b_process_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(CaptureDesc), ctypes.c_size_t]
    L.sora_rx11b_process.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(CaptureDesc), ctypes.c_size_t]
    _res_of = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(FrameResult), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p, ctypes.c_size_t]
    _deliver = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.sora_ht40_process_captures_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32]
    L.sora_ht40_soft_of.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.sora_ht40_found_of.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.sora_rx_stream_record_of.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    # what the four receive handles share (include/sora_hip.h: tickets, calls in flight, stream continuation)
    vp = ctypes.c_void_p
    shared = [("_destroy", [vp], None), ("_stream", [vp], vp), ("_ticket", [vp], ctypes.c_int), ("_wait", [vp, ctypes.c_int], ctypes.c_int),
              ("_wait_any", [vp, ctypes.POINTER(ctypes.c_int)], ctypes.c_int), ("_stream_of", [vp, ctypes.c_int], vp), ("_results_of", _res_of, ctypes.c_int),
              ("_deliver_async", _deliver, ctypes.c_int), ("_synchronize", [vp], ctypes.c_int), ("_calls_in_flight", [vp], ctypes.c_int),
              ("_set_stream_mode", [vp, ctypes.c_int], ctypes.c_int), ("_stream_consumed", [vp, ctypes.c_int, vp, ctypes.c_size_t], ctypes.c_int)]
    for pre in ("sora_rx", "sora_rx11b", "sora_rx11n", "sora_ht40"):
        for suffix, args, res in shared:
            if pre + suffix in EXPORTS:
                f = getattr(L, pre + suffix); f.argtypes = args; f.restype = res
    L.sora_rx11b_results.argtypes = [ctypes.c_void_p, ctypes.POINTER(FrameResult), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                     ctypes.c_void_p, ctypes.c_size_t]
    _lib = L
    return L


def _check(rc):
    if rc != SORA_OK:
        raise SoraError(rc, (load().sora_hip_last_error() or b"").decode())


def device_count():
    return load().sora_hip_device_count()


def _dev_ptr(x):
    """Device pointer of a torch CUDA tensor (or an int address)."""
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        if not x.is_cuda:
            raise ValueError("expected a device (HBM) tensor")
        if not x.is_contiguous():
            raise ValueError("expected a contiguous tensor")
        return x.data_ptr()
    raise TypeError("expected a torch CUDA tensor or an integer device address")


class _Handle:
    """What the four receive handles share (include/sora_hip.h): their calls in flight -- tickets, wait, wait_any, deliver_async --, stream
    continuation, and the step from a FrameResult table to dicts.  _pre: the prefix of the handle's C entry points."""
    _pre = ""
    _h = None

    def _c(self, suffix):
        return getattr(self._L, self._pre + suffix)

    def close(self):
        if self._h:
            self._c("_destroy")(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def ticket(self):
        """ticket of the most recent process call (0: none)"""
        return self._c("_ticket")(self._h)

    def wait(self, ticket):
        _check(self._c("_wait")(self._h, int(ticket)))

    def wait_any(self):
        """Block until some call with an enqueued delivery (deliver_async) has finished -> its ticket (the oldest finished one).  The call is then
        released: the next process call may reuse its slot ahead of older calls still in flight."""
        t = ctypes.c_int(0)
        _check(self._c("_wait_any")(self._h, ctypes.byref(t)))
        return t.value

    def deliver_async(self, ticket, buf):
        """Enqueue the delivery of the call's rows (+ MPDU array when buf.mpdu is not None) into the page-locked HostResults `buf`, behind the
        call's kernels; valid after wait(ticket).  (buf.counts and buf.nrows start at the same address.)"""
        _check(self._c("_deliver_async")(self._h, int(ticket), buf.rows.ctypes.data, len(buf.rows), buf.counts.ctypes.data,
                                         buf.mpdu.ctypes.data if buf.mpdu is not None else None, buf.mpdu.size if buf.mpdu is not None else 0))

    def set_stream_mode(self, enable=-1):
        """1: capture k of a call continues capture k of the call before it (sora_hip.h: stream continuation); returns the previous mode"""
        r = int(self._c("_set_stream_mode")(self._h, int(enable)))
        if r not in (0, 1):
            raise SoraError(r, (self._L.sora_hip_last_error() or b"").decode())
        return r

    def stream_consumed(self, ticket, ncaps):
        """per capture of the most recent call: input-rate samples that are final = where the next call's capture must start in the stream"""
        out = np.zeros(ncaps, np.uint32)
        _check(self._c("_stream_consumed")(self._h, int(ticket), out.ctypes.data, int(ncaps)))
        return out

    @staticmethod
    def _table(res, n, mp, every_row=False):
        """the first n FrameResult rows -> dicts; "mpdu": the row's bytes of mp (rows with E_FRAME_OK / E_CRC32_FAIL, or every row), no key if mp is None"""
        out = []
        for r in res[:n]:
            d = {f: getattr(r, f) for f, _ in FrameResult._fields_}
            if mp is not None:
                has = every_row or r.error_code in (E_FRAME_OK, E_CRC32_FAIL)
                d["mpdu"] = mp[r.mpdu_offset:r.mpdu_offset + min(r.length, 4096)].tobytes() if has else b""
            out.append(d)
        return out


class Rx(_Handle):
    """sora_rx_t: the 802.11a demod graph over a batch of captures."""
    _pre = "sora_rx"

    def __init__(self, max_captures, max_total_samples, sample_rate_mhz=20, device=0, max_frames_per_capture=2,
                 cca_pwr_threshold=0):
        L = load()
        cfg = RxCfg(ctypes.sizeof(RxCfg), device, sample_rate_mhz, max_captures, max_total_samples,
                    max_frames_per_capture, cca_pwr_threshold)
        h = ctypes.c_void_p()
        _check(L.sora_rx_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h; self._L = L; self.cfg = cfg; self._keep = None
        self.wait_for_producer = True      # process_dev first waits for torch's current stream (bench.py turns it off: its inputs are resident)
        # harness-side overrides (the library itself reads no environment variable): A/B runs of the tools and tests
        if os.environ.get("SORA_HIP_DEPTH"): self.set_depth(int(os.environ["SORA_HIP_DEPTH"]))
        if os.environ.get("SORA_HIP_GRAPH"): self.set_graph(int(os.environ["SORA_HIP_GRAPH"]))
        if os.environ.get("SORA_HIP_TRELLIS"): self.set_trellis(int(os.environ["SORA_HIP_TRELLIS"]))
        if os.environ.get("SORA_HIP_FRONT"): self.set_front(int(os.environ["SORA_HIP_FRONT"]))

    @property
    def stream(self):
        return self._L.sora_rx_stream(self._h)

    CAPTURE_DTYPE = np.dtype([("offset", "<u8"), ("nsamples", "<u4"), ("capture_id", "<u4")])   # = sora_capture_desc

    @classmethod
    def captures(cls, captures):
        """[(offset, nsamples[, id])] -> packed sora_capture_desc array (build it once when the same set is submitted repeatedly)."""
        if isinstance(captures, np.ndarray) and captures.dtype == cls.CAPTURE_DTYPE:
            return np.ascontiguousarray(captures)
        arr = np.zeros(len(captures), cls.CAPTURE_DTYPE)
        if len(captures):
            if all(len(c) > 2 for c in captures):
                a = np.asarray(captures, dtype=np.uint64).reshape(len(captures), -1)
                arr["offset"] = a[:, 0]; arr["nsamples"] = a[:, 1]; arr["capture_id"] = a[:, 2]
            else:
                for i, c in enumerate(captures):
                    arr[i] = (c[0], c[1], c[2] if len(c) > 2 else i)
        return arr

    @classmethod
    def _caps(cls, captures):
        arr = cls.captures(captures)
        return arr, arr.ctypes.data_as(ctypes.POINTER(CaptureDesc))

    def process_dev(self, d_iq, captures):
        """d_iq: int16 torch CUDA tensor [N,2] (resident in HBM); captures: [(offset, nsamples[, id])]."""
        arr, ptr = self._caps(captures)
        _hold(self, d_iq)
        _check(self._L.sora_rx_process_dev(self._h, _dev_ptr(d_iq), ptr, len(arr)))
        return self.ticket()

    def process(self, h_iq, captures):
        a = np.ascontiguousarray(h_iq, np.int16).reshape(-1, 2)
        arr, ptr = self._caps(captures)
        _check(self._L.sora_rx_process(self._h, a.ctypes.data, len(a), ptr, len(arr)))
        return self.ticket()

    def process_dump(self, h_dump, flags, captures):
        """h_dump: the raw dump bytes in host memory -- a numpy uint8 array or a (pinned) torch CPU uint8 tensor, untouched until the call has
        completed; flags: INGEST_*; captures address the ingested stream.  Copy, ingest and the receive chain run on the call's own stream."""
        arr, ptr = self._caps(captures)
        if hasattr(h_dump, "data_ptr"):
            addr, nbytes = h_dump.data_ptr(), h_dump.numel() * h_dump.element_size()
        else:
            a = np.ascontiguousarray(h_dump).view(np.uint8).reshape(-1); addr, nbytes = a.ctypes.data, a.size; h_dump = a
        if self._keep is None:
            self._keep = collections.deque(maxlen=17)
        self._keep.append(h_dump)
        _check(self._L.sora_rx_process_dump(self._h, ctypes.c_void_p(addr), nbytes, int(flags), ptr, len(arr)))
        return self.ticket()

    def mpdu_bytes(self, ticket):
        return int(self._L.sora_rx_mpdu_bytes(self._h, int(ticket)))

    def results_dev(self, ticket=None):
        """Device-resident results of the last call (or of the call `ticket` names): (rows int32 tensor [cap_rows, 9] (36-byte
        sora_frame_result rows), nrows int32 tensor [1], mpdu uint8 base address).  The tensors alias library memory: valid
        until that pipeline's next call."""
        import torch
        rows = ctypes.c_void_p(); nrows = ctypes.c_void_p(); mpdu = ctypes.c_void_p()
        if ticket is None:
            _check(self._L.sora_rx_results_dev(self._h, ctypes.byref(rows), ctypes.byref(nrows), ctypes.byref(mpdu)))
        else:
            _check(self._L.sora_rx_results_dev_of(self._h, int(ticket), ctypes.byref(rows), ctypes.byref(nrows), ctypes.byref(mpdu)))
        cap = self.cfg.max_captures * self.cfg.max_frames_per_capture
        dev = torch.device("cuda", self.cfg.device)

        class _Arr:                                        # __cuda_array_interface__ view over library memory
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}
        r = torch.as_tensor(_Arr(rows.value, (cap, 9), "<i4"), device=dev)
        n = torch.as_tensor(_Arr(nrows.value, (1,), "<i4"), device=dev)
        return r, n, mpdu.value

    def set_profiling(self, enable=True):
        _check(self._L.sora_rx_set_profiling(self._h, 1 if enable else 0))

    def set_depth(self, depth=0):
        """number of process calls kept in flight on internal pipelines (1..8); returns the previous value"""
        return int(self._L.sora_rx_set_depth(self._h, int(depth)))

    def set_trellis(self, lanes_per_pair=-1):
        """64: k_viterbi, 16: k_viterbi16, 1 (TRELLIS_WINDOWED): k_viterbi16w, 0: the library chooses from the capacity in flight; returns the previous setting"""
        r = int(self._L.sora_rx_set_trellis(self._h, int(lanes_per_pair)))
        if r < 0: _check(r)
        return r

    def set_front(self, kernels=-1):
        """1: k_frame (one wave per frame), 3: k_sym_front -> k_track_lds -> k_sym_back, 4: k_pipe (those and the window-parallel trellis as one launch),
        0: the library chooses; returns the previous setting"""
        r = int(self._L.sora_rx_set_front(self._h, int(kernels)))
        if r < 0: _check(r)
        return r

    def front(self):
        return int(self._L.sora_rx_front(self._h))

    def stream_record_of(self, ticket, capture):
        """sora_rx_stream_record_of: the 64 words of capture `capture`'s continuation record after the most recent call (a diagnostic; stream mode only)"""
        out = np.zeros(64, np.uint32); n = ctypes.c_size_t(0)
        _check(self._L.sora_rx_stream_record_of(self._h, int(ticket), int(capture), out.ctypes.data, out.size, ctypes.byref(n)))
        return out[:n.value]

    def set_ordered(self, on=-1):
        """1: calls in flight complete in submission order (a call's trellis kernel starts behind the previous call's); returns the previous setting"""
        r = int(self._L.sora_rx_set_ordered(self._h, int(on)))
        if r < 0: _check(r)
        return r

    def call_front(self, ticket=0):
        """the kernels call `ticket` (0: the most recent one) WAS launched with -- latched at its process call, where front() is a forecast"""
        r = int(self._L.sora_rx_call_front(self._h, int(ticket)))
        if r < 0: _check(r)
        return r

    def trellis(self):
        """lanes per frame pair of the trellis kernel the next call uses (64: k_viterbi, 16: k_viterbi16, 1 = TRELLIS_WINDOWED: k_viterbi16w)"""
        return int(self._L.sora_rx_trellis(self._h))

    def window_stats(self):
        """the window-parallel trellis's proof record since the handle was created (waits for the calls in flight)"""
        v = (ctypes.c_ulonglong * 4)()
        _check(self._L.sora_rx_window_stats(self._h, v))
        return {"boundaries": int(v[0]), "boundaries_failed": int(v[1]), "frames_decoded_again": int(v[2]), "units": int(v[3])}

    def bind_mpdu(self, buf):
        """the NEXT process call writes its MPDUs straight into the page-locked HostResults `buf` (deliver_async(ticket, buf) then copies rows and count only); None cancels"""
        if buf is None:
            _check(self._L.sora_rx_bind_mpdu(self._h, None, 0))
        else:
            _check(self._L.sora_rx_bind_mpdu(self._h, buf.mpdu.ctypes.data, buf.mpdu.size))

    def set_pipe_wait_us(self, us=-1):
        """bound of the waits inside a k_pipe launch (0: every wait that is not satisfied at once gives up -> the call is made again by the finishing kernel)"""
        return int(self._L.sora_rx_set_pipe_wait_us(self._h, int(us)))

    def pipe_stats(self):
        """k_pipe's safety net since the handle was created (waits for the calls in flight)"""
        v = (ctypes.c_ulonglong * 2)()
        _check(self._L.sora_rx_pipe_stats(self._h, v))
        return {"calls_made_again": int(v[0]), "backoffs": int(v[1])}

    def set_graph(self, enable=-1):
        return int(self._L.sora_rx_set_graph(self._h, int(enable)))

    def set_fused(self, enable=-1):
        """The fused data-field kernel (k_decode) has been removed: 1 raises SoraError SORA_E_NOT_SUPPORTED, 0 and the query (-1) return 0"""
        r = int(self._L.sora_rx_set_fused(self._h, int(enable)))
        if r not in (0, 1):
            raise SoraError(r, (self._L.sora_hip_last_error() or b"").decode())
        return r

    def kernel_times(self):
        """{kernel name: ms} of the profiled process calls (HIP events on the handle's streams)."""
        ms = (ctypes.c_float * 8)(); n = ctypes.c_size_t(0)
        _check(self._L.sora_rx_kernel_times(self._h, ms, 8, ctypes.byref(n)))
        name = self._L.sora_rx_kernel_name
        return {name(i).decode(): ms[i] for i in range(n.value) if name(i)}

    def flush(self):
        _check(self._L.sora_rx_flush(self._h))

    def reset(self):
        _check(self._L.sora_rx_reset(self._h))

    def results(self, with_mpdu=True, max_frames=None, ticket=None):
        """Frames of the most recent process call, or of the call `ticket` names."""
        if max_frames is None:
            max_frames = self.cfg.max_captures * self.cfg.max_frames_per_capture
        res = (FrameResult * max(1, max_frames))()
        n = ctypes.c_size_t(0)
        mp = np.zeros(max_frames * 2504 if with_mpdu else 1, np.uint8)
        if ticket is None:
            _check(self._L.sora_rx_results(self._h, res, max_frames, ctypes.byref(n), mp.ctypes.data if with_mpdu else None, mp.size))
        else:
            _check(self._L.sora_rx_results_of(self._h, int(ticket), res, max_frames, ctypes.byref(n), mp.ctypes.data if with_mpdu else None, mp.size))
        return self._table(res, n.value, mp if with_mpdu else None)


ROW_DTYPE = np.dtype([("capture_id", "<u4"), ("start_sample", "<u4"), ("end_sample", "<u4"), ("error_code", "<u4"), ("rate_kbps", "<u4"),
                      ("length", "<u2"), ("nsym", "<u2"), ("crc32", "<u4"), ("cfo_est", "<i2"), ("flags", "<u2"), ("mpdu_offset", "<u4")])   # = sora_frame_result
ROW_TRUNCATED = 1
ROW_SHORT_PREAMBLE = 2        # an 802.11b row whose frame came behind the short preamble (Rx11b.set_preamble(1))
ROW_SHORT_GI = 4              # a 40 MHz HT row whose frame had the short guard interval (SORA_ROW_SHORT_GI)
HT40_SHORT_GI = 0x100         # SORA_HT40_SHORT_GI: on a descriptor's code rate (in) and on a found record's mcs (out)
HT40_GUARD_LONG, HT40_GUARD_SIGNALLED = 0, 1


class HostResults:
    """Page-locked host buffers for Rx.deliver_async: rows (ROW_DTYPE), nrows (uint32[1]) and, optionally, the MPDU array
    (row["mpdu_offset"] indexes it).  Memory comes from sora_hip_host_alloc; close() releases it."""

    def __init__(self, max_rows, mpdu_bytes=0):
        L = load()
        self._L = L
        assert ROW_DTYPE.itemsize == ctypes.sizeof(FrameResult) == 36
        sizes = [max(1, max_rows) * 36, 64, max(0, int(mpdu_bytes))]
        self._ptrs = []
        arrs = []
        for nbytes in sizes:
            if nbytes == 0:
                arrs.append(None); continue
            p = L.sora_hip_host_alloc(nbytes)
            if not p:
                raise SoraError(-1, "sora_hip_host_alloc failed")
            self._ptrs.append(p)
            arrs.append(np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p)))
        self.rows = arrs[0].view(ROW_DTYPE)
        self.nrows = arrs[1][:4].view(np.uint32)
        self.counts = arrs[1][:8].view(np.uint32)       # the 11b / 11n / HT40 handles deliver {rows, MPDU bytes}
        self.mpdu = arrs[2]

    def results(self):
        """the delivered table as the list of dicts Rx*.results() returns (after wait(ticket)): dense MPDUs, mpdu_offset indexes self.mpdu"""
        out = []
        for r in self.rows[:int(self.counts[0])]:
            d = {k: int(r[k]) for k in ROW_DTYPE.names}
            has = d["error_code"] in (E_FRAME_OK, E_CRC32_FAIL) and self.mpdu is not None
            d["mpdu"] = self.mpdu[d["mpdu_offset"]:d["mpdu_offset"] + min(d["length"], 4096)].tobytes() if has else b""
            d["stream"] = d["start_sample"]
            out.append(d)
        return out

    def close(self):
        for p in self._ptrs:
            self._L.sora_hip_host_free(p)
        self._ptrs = []
        self.rows = self.nrows = self.mpdu = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Rx11b(_Handle):
    """sora_rx11b_t: the 802.11b demod graph (44 MHz samples) over a batch of captures."""
    _pre = "sora_rx11b"

    def __init__(self, max_captures, max_total_samples, device=0, max_frames_per_capture=8, cca_pwr_threshold=0):
        L = load()
        cfg = RxCfg(ctypes.sizeof(RxCfg), device, 44, max_captures, max_total_samples, max_frames_per_capture, cca_pwr_threshold)
        h = ctypes.c_void_p()
        _check(L.sora_rx11b_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h; self._L = L; self.cfg = cfg; self._keep = None

    def synchronize(self):
        _check(self._L.sora_rx11b_synchronize(self._h))

    def process_dev(self, d_iq, captures):
        arr, ptr = Rx._caps(captures)
        _hold(self, d_iq)
        _check(self._L.sora_rx11b_process_dev(self._h, _dev_ptr(d_iq), ptr, len(arr)))
        return self.ticket()

    def calls_in_flight(self):
        return int(self._L.sora_rx11b_calls_in_flight(self._h))

    def set_single_pass(self, enable=-1):
        """the pass plan: 2 automatic (default), 1 every capture straight through the CCK-capable kernel, 0 always two passes; returns the previous plan"""
        return int(self._L.sora_rx11b_set_single_pass(self._h, int(enable)))

    def set_preamble(self, mode=-1):
        """which preambles TSFDSync accepts: 0 long only (default, the reference's graph), 1 long and short (rows of short-preamble frames carry
        ROW_SHORT_PREAMBLE in "flags"); negative: query.  Waits for the calls in flight.  Returns the previous mode."""
        r = int(self._L.sora_rx11b_set_preamble(self._h, int(mode)))
        if r < 0: _check(r)
        return r

    def process(self, h_iq, captures):
        a = np.ascontiguousarray(h_iq, np.int16).reshape(-1, 2)
        arr, ptr = Rx._caps(captures)
        _check(self._L.sora_rx11b_process(self._h, a.ctypes.data, len(a), ptr, len(arr)))

    def results(self, ticket=None, with_mpdu=True):
        max_frames = self.cfg.max_captures * self.cfg.max_frames_per_capture
        res = (FrameResult * max(1, max_frames))()
        n = ctypes.c_size_t(0)
        mp = np.zeros(max_frames * 4096 if with_mpdu else 1, np.uint8)
        if ticket is None:
            _check(self._L.sora_rx11b_results(self._h, res, max_frames, ctypes.byref(n), mp.ctypes.data if with_mpdu else None, mp.size))
        else:
            _check(self._L.sora_rx11b_results_of(self._h, int(ticket), res, max_frames, ctypes.byref(n), mp.ctypes.data if with_mpdu else None, mp.size))
        return self._table(res, n.value, mp if with_mpdu else mp[:0])        # (without MPDUs every row's "mpdu" is b"")


class Rx11n(_Handle):
    """sora_rx11n_t: the 802.11n 2x2 demod graph (two RX chains at 40 MHz) over a batch of captures; rate_kbps = MCS index."""
    _pre = "sora_rx11n"

    def __init__(self, max_captures, max_total_samples, device=0, max_frames_per_capture=8):
        L = load()
        cfg = RxCfg(ctypes.sizeof(RxCfg), device, 40, max_captures, max_total_samples, max_frames_per_capture, 0)
        h = ctypes.c_void_p()
        _check(L.sora_rx11n_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h; self._L = L; self.cfg = cfg; self._keep = None

    def synchronize(self):
        """waits for every call in flight"""
        _check(self._L.sora_rx11n_synchronize(self._h))

    def set_depth(self, depth=0):
        r = self._L.sora_rx11n_set_depth(self._h, depth)
        if r < 0: _check(r)
        return r

    def set_trellis(self, lanes_per_pair=-1):
        r = int(self._L.sora_rx11n_set_trellis(self._h, int(lanes_per_pair)))
        if r < 0: _check(r)
        return r

    def trellis(self):
        """the trellis kernel the next call uses: 64, 16 or 1 (TRELLIS_WINDOWED)"""
        return int(self._L.sora_rx11n_trellis(self._h))

    def set_mcs_max(self, mcs_max=-1):
        """the highest MCS the SIG parser accepts: 10 (default: the reference's gate) .. 14; returns the previous value (sora_hip.h: sora_rx11n_set_mcs_max)"""
        r = int(self._L.sora_rx11n_set_mcs_max(self._h, int(mcs_max)))
        if r < 0: _check(r)
        return r

    def window_stats(self):
        v = (ctypes.c_ulonglong * 4)()
        _check(self._L.sora_rx11n_window_stats(self._h, v))
        return {"boundaries": int(v[0]), "boundaries_failed": int(v[1]), "frames_decoded_again": int(v[2]), "units": int(v[3])}

    def process_dev(self, d_iq0, d_iq1, captures):
        arr, ptr = Rx._caps(captures)
        _hold(self, (d_iq0, d_iq1))
        _check(self._L.sora_rx11n_process_dev(self._h, _dev_ptr(d_iq0), _dev_ptr(d_iq1), ptr, len(arr)))
        return self.ticket()

    def process(self, h_iq0, h_iq1, captures):
        a = np.ascontiguousarray(h_iq0, np.int16).reshape(-1, 2); b = np.ascontiguousarray(h_iq1, np.int16).reshape(-1, 2)
        assert len(a) == len(b)
        arr, ptr = Rx._caps(captures)
        _check(self._L.sora_rx11n_process(self._h, a.ctypes.data, b.ctypes.data, len(a), ptr, len(arr)))

    def results(self, ticket=None):
        max_frames = self.cfg.max_captures * self.cfg.max_frames_per_capture
        res = (FrameResult * max(1, max_frames))()
        n = ctypes.c_size_t(0)
        mp = np.zeros(max_frames * 4096, np.uint8)
        if ticket is None:
            _check(self._L.sora_rx11n_results(self._h, res, max_frames, ctypes.byref(n), mp.ctypes.data, mp.size))
        else:
            _check(self._L.sora_rx11n_results_of(self._h, int(ticket), res, max_frames, ctypes.byref(n), mp.ctypes.data, mp.size))
        return self._table(res, n.value, mp)


class RxHt40(_Handle):
    """sora_ht40_t: the data field of HT-mixed 40 MHz two-stream frames (BASELINE configs[3]; parity unpinned, see include/sora_hip.h).  set_stream_mode /
    stream_consumed (the shared ones above) apply to process_captures_dev: a stream-mode call takes at most max_frames captures."""
    _pre = "sora_ht40"

    def __init__(self, max_frames, max_soft_values, device=0):
        L = load()
        h = ctypes.c_void_p()
        _check(L.sora_ht40_create(device, max_frames, max_soft_values, ctypes.byref(h)))
        self._h = h; self._L = L; self.max_frames = max_frames; self._keep = None

    def synchronize(self):
        _check(self._L.sora_ht40_synchronize(self._h))

    @staticmethod
    def frames(descs):
        """[(offset, n_bpsc, code_rate, length0, length1, cfo, noise_var[, id])] -> packed descriptor array (reusable); code_rate may carry HT40_SHORT_GI"""
        if isinstance(descs, ctypes.Array):
            return descs
        arr = (Ht40Frame * max(1, len(descs)))()
        for i, d in enumerate(descs):
            arr[i].offset = d[0]; arr[i].n_bpsc = d[1]; arr[i].code_rate = d[2]; arr[i].length[0] = d[3]; arr[i].length[1] = d[4]
            arr[i].cfo = d[5]; arr[i].noise_var = d[6]; arr[i].frame_id = d[7] if len(d) > 7 else i
        arr._n = len(descs)
        return arr

    def set_trellis(self, lanes_per_pair=-1):
        r = int(self._L.sora_ht40_set_trellis(self._h, int(lanes_per_pair)))
        if r < 0: _check(r)
        return r

    def set_coding(self, coding=-1):
        """sora_ht40_set_coding: CODING_PER_STREAM (0, the default) or CODING_JOINT (1: one PSDU per frame, stream-parsed; descriptors carry l1 = 0, one row per
        frame, soft(frame, 0) is the merged stream).  -> the previous value; a negative argument only queries"""
        r = int(self._L.sora_ht40_set_coding(self._h, int(coding)))
        if r < 0: _check(r)
        return r

    def set_guard(self, mode=-1):
        """sora_ht40_set_guard: HT40_GUARD_LONG (0, the default: HT-SIG's Short GI bit is not looked at) or HT40_GUARD_SIGNALLED (1: the front end of
        process_captures_dev reads it; the rows of a short-GI frame carry ROW_SHORT_GI).  -> the previous mode; a negative argument only queries"""
        r = int(self._L.sora_ht40_set_guard(self._h, int(mode)))
        if r < 0: _check(r)
        return r

    def set_mcs_max(self, mcs_max=0):
        """sora_ht40_set_mcs_max: 14 (the default) or 15 (descriptors may carry CR_56, the front end of process_captures_dev admits MCS 15; such frames are decoded by
        k_viterbi56_11n).  -> the previous value; an argument <= 0 only queries"""
        r = int(self._L.sora_ht40_set_mcs_max(self._h, int(mcs_max)))
        if r < 0: _check(r)
        return r

    def process_dev(self, d_iq0, d_iq1, descs, d_weights=None):
        arr = self.frames(descs); n = getattr(arr, "_n", len(arr))
        _hold(self, (d_iq0, d_iq1, d_weights)); self._n = n
        _check(self._L.sora_ht40_process_dev(self._h, _dev_ptr(d_iq0), _dev_ptr(d_iq1), arr, n, _dev_ptr(d_weights) if d_weights is not None else None))
        t = self.ticket()
        self._nof = getattr(self, "_nof", {}); self._nof[t] = n
        self._prune_nof()
        return t

    def _prune_nof(self):
        """forget the row bounds of tickets the LIBRARY no longer knows (a released slot is reused ahead of older calls still in flight, so ticket arithmetic
        does not tell: ADVICE r4)"""
        for old in [k for k in self._nof if not self._L.sora_ht40_stream_of(self._h, int(k))]:
            del self._nof[old]

    def process_captures_dev(self, d_iq0, d_iq1, captures, max_frames_per_capture=4):
        """raw two-chain 40 MHz captures [(offset, nsamples[, id])]: the front end finds, parses and measures the frames"""
        arr, ptr = Rx._caps(captures)
        _hold(self, (d_iq0, d_iq1))
        _check(self._L.sora_ht40_process_captures_dev(self._h, _dev_ptr(d_iq0), _dev_ptr(d_iq1), ptr, len(arr), int(max_frames_per_capture)))
        t = self.ticket()
        self._n = len(arr) * int(max_frames_per_capture)
        self._nof = getattr(self, "_nof", {}); self._nof[t] = self._n
        self._prune_nof()
        return t

    def calls_in_flight(self):
        return int(self._L.sora_ht40_calls_in_flight(self._h))

    def results(self, with_mpdu=True, ticket=None):
        n2 = 2 * (self._n if ticket is None else self._nof.get(int(ticket), self.max_frames))
        res = (FrameResult * max(1, n2))(); n = ctypes.c_size_t(0)
        mp = np.zeros(n2 * 4096 if with_mpdu else 1, np.uint8)
        if ticket is None:
            _check(self._L.sora_ht40_results(self._h, res, n2, ctypes.byref(n), mp.ctypes.data if with_mpdu else None, mp.size))
        else:
            _check(self._L.sora_ht40_results_of(self._h, int(ticket), res, n2, ctypes.byref(n), mp.ctypes.data if with_mpdu else None, mp.size))
        out = self._table(res, n.value, mp if with_mpdu else None, every_row=True)
        for d in out:
            d["stream"] = d["start_sample"]; d["short_gi"] = bool(d["flags"] & ROW_SHORT_GI)
        return out

    def soft(self, frame, stream, ticket=None):
        """sora_ht40_soft_of: the de-interleaved soft bytes (uint8 [nsym * 108 * n_bpsc]) of spatial stream `stream` of described frame `frame` of a process_dev call
        (ticket None: the most recent call) -- a diagnostic for tests"""
        t = self.ticket() if ticket is None else int(ticket)
        n = ctypes.c_size_t(0)
        rc = self._L.sora_ht40_soft_of(self._h, t, int(frame), int(stream), None, 0, ctypes.byref(n))
        if rc != SORA_OK and n.value == 0:
            _check(rc)
        out = np.zeros(n.value, np.uint8)
        _check(self._L.sora_ht40_soft_of(self._h, t, int(frame), int(stream), out.ctypes.data, out.size, ctypes.byref(n)))
        return out[:n.value]

    def found(self, capture, ticket=None):
        """sora_ht40_found_of: the front end's records of capture `capture` (index into the call's captures) of a process_captures_dev call (ticket None: the most
        recent call), in time order: [{a20, mcs, ht_len, nsym, cfo, noise_var (numpy float32), end_sample, error_code}] -- a diagnostic for tests; mcs carries
        HT40_SHORT_GI for a recorded short-GI frame (set_guard(1))"""
        t = self.ticket() if ticket is None else int(ticket)
        n = ctypes.c_size_t(0)
        rc = self._L.sora_ht40_found_of(self._h, t, int(capture), None, 0, ctypes.byref(n))
        if rc != SORA_OK and n.value == 0:
            _check(rc)
        arr = (Ht40Found * max(1, n.value))()
        _check(self._L.sora_ht40_found_of(self._h, t, int(capture), arr, n.value, ctypes.byref(n)))
        return [{"a20": r.a20, "mcs": r.mcs, "ht_len": r.ht_len, "nsym": r.nsym, "cfo": r.cfo, "noise_var": np.float32(r.noise_var), "end_sample": r.end_sample,
                 "error_code": r.error_code} for r in arr[:n.value]]


def ht40_symbols(length0, length1, n_bpsc, code_rate):
    return load().sora_ht40_symbols(length0, length1, n_bpsc, code_rate)


HT40_CODING_PER_STREAM, HT40_CODING_JOINT = 0, 1


def ht40_symbols_joint(length, n_bpsc, code_rate):
    """data symbols of a joint-coded 40 MHz HT frame whose one PSDU has `length` bytes (sora_ht40_symbols_joint; 0: bad arguments)"""
    return int(load().sora_ht40_symbols_joint(int(length), int(n_bpsc), int(code_rate)))


# ---- per-stage entry points on torch CUDA tensors ---------------------------------------------------
def _hold(obj, item, sync=True):
    """The handles keep several calls in flight on their own non-blocking streams (up to 16: sora_rx_set_depth): (i) the inputs of the last 17 calls stay referenced
    (torch's caching allocator must not hand a block to the next tensor while a kernel still reads it), (ii) whatever produced the
    tensors on torch's current stream has finished before the library's stream reads them."""
    import collections
    if getattr(obj, "_keep", None) is None:
        obj._keep = collections.deque(maxlen=17)
    obj._keep.append(item)
    if sync and getattr(obj, "wait_for_producer", True):
        import torch
        torch.cuda.current_stream().synchronize()


def _stream_ptr(stream):
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return stream


def fft64(x, stream=None):
    """TFFT64: x int16 CUDA tensor [n,64,2] -> same shape."""
    import torch
    out = torch.empty_like(x)
    _check(load().sora_hip_fft64(_dev_ptr(x), _dev_ptr(out), x.shape[0], _stream_ptr(stream)))
    return out


def fft128(x, stream=None):
    """FFT<128>: x int16 CUDA tensor [n,128,2] -> same shape."""
    import torch
    out = torch.empty_like(x)
    _check(load().sora_hip_fft128(_dev_ptr(x), _dev_ptr(out), x.shape[0], _stream_ptr(stream)))
    return out


def lts11a(x, stream=None):
    """T11aLTS: x int16 CUDA [n,144,2] -> int16 CUDA [n,258]: (cfo_est, reserved, freq[64][2], chan[64][2])."""
    import torch
    out = torch.zeros((x.shape[0], 258), dtype=torch.int16, device=x.device)
    _check(load().sora_hip_lts11a(_dev_ptr(x), _dev_ptr(out), x.shape[0], _stream_ptr(stream)))
    return out


def symfront11a(x, ctx, ctx_index=None, stream=None):
    """x int16 CUDA [n,80,2], ctx = lts11a() output [m,258], ctx_index int32 CUDA [n] or None -> eq int16 [n,64,2]."""
    import torch
    out = torch.empty((x.shape[0], 64, 2), dtype=torch.int16, device=x.device)
    _check(load().sora_hip_symfront11a(_dev_ptr(x), _dev_ptr(ctx), _dev_ptr(ctx_index) if ctx_index is not None else None,
                                       _dev_ptr(out), x.shape[0], _stream_ptr(stream)))
    return out


def _cmul64(fn, x, coef, index, stream):
    import torch
    out = torch.empty_like(x)
    _check(getattr(load(), fn)(_dev_ptr(x), _dev_ptr(coef), _dev_ptr(index) if index is not None else None, _dev_ptr(out), x.shape[0], _stream_ptr(stream)))
    return out


def freq_comp11a(x, ctx, ctx_index=None, stream=None):
    """TFreqCompensation alone: x int16 CUDA [n,64,2], ctx = lts11a() output [m,258], ctx_index int32 CUDA [n] or None -> [n,64,2]"""
    return _cmul64("sora_hip_freq_comp11a", x, ctx, ctx_index, stream)


def equalize11a(x, ctx, ctx_index=None, stream=None):
    """TChannelEqualization alone (same arguments)"""
    return _cmul64("sora_hip_equalize11a", x, ctx, ctx_index, stream)


def phase_comp11a(x, state, state_index=None, stream=None):
    """TPhaseCompensate alone: state int16 CUDA [m,134] (sora_track11a_state), state_index int32 CUDA [n] or None"""
    return _cmul64("sora_hip_phase_comp11a", x, state, state_index, stream)


def pilot_track11a(eq, first, nsym, state, stream=None):
    """eq int16 CUDA [total,64,2]; first/nsym int32 CUDA [f]; state int16 CUDA [f,134] (in/out) -> tracked [total,64,2]."""
    import torch
    out = torch.zeros_like(eq)
    _check(load().sora_hip_pilot_track11a(_dev_ptr(eq), _dev_ptr(first), _dev_ptr(nsym), _dev_ptr(state), _dev_ptr(out), first.shape[0], _stream_ptr(stream)))
    return out


def set_share_window_us(us):
    """the window in which another batch-sized handle's call makes a small handle's automatic choice leave k_pipe alone (process-wide; returns the old value)"""
    return int(load().sora_hip_set_share_window_us(int(us)))


def pilot11a(x, first, nsym, state, stream=None):
    """TPilotTrack alone: x = TPhaseCompensate's output, int16 CUDA [total,64,2]; the frame tables and the state of pilot_track11a."""
    import torch
    out = torch.zeros_like(x)
    _check(load().sora_hip_pilot11a(_dev_ptr(x), _dev_ptr(first), _dev_ptr(nsym), _dev_ptr(state), _dev_ptr(out), first.shape[0], _stream_ptr(stream)))
    return out


def demap11a(x, n_bpsc, stream=None):
    import torch
    out = torch.empty((x.shape[0], 48 * n_bpsc), dtype=torch.uint8, device=x.device)
    _check(load().sora_hip_demap11a(_dev_ptr(x), _dev_ptr(out), n_bpsc, x.shape[0], _stream_ptr(stream)))
    return out


def demap11n(x, n_bpsc, stream=None):
    """x: int16 CUDA tensor [n,64,2] (pilot-tracked symbols of one spatial stream) -> uint8 [n, 52*n_bpsc]."""
    import torch
    out = torch.empty((x.shape[0], 52 * n_bpsc), dtype=torch.uint8, device=x.device)
    _check(load().sora_hip_demap11n(_dev_ptr(x), _dev_ptr(out), n_bpsc, x.shape[0], _stream_ptr(stream)))
    return out


def deinterleave11n(s, n_bpsc, spatial_stream, stream=None):
    """s: uint8 CUDA tensor [n, 52*n_bpsc] of spatial stream 0 or 1 -> de-interleaved, same shape."""
    import torch
    out = torch.empty_like(s)
    _check(load().sora_hip_deinterleave11n(_dev_ptr(s), _dev_ptr(out), n_bpsc, spatial_stream, s.shape[0], _stream_ptr(stream)))
    return out


def cfo_est11n(lltf0, lltf1, stream=None):
    """lltf0/lltf1: int16 CUDA [n,128,2] -> state int16 CUDA [n,24] (vfo_delta_i | vfo_step_i | vfo_theta_i)."""
    import torch
    st = torch.empty((lltf0.shape[0], 24), dtype=torch.int16, device=lltf0.device)
    _check(load().sora_hip_cfo_est11n(_dev_ptr(lltf0), _dev_ptr(lltf1), _dev_ptr(st), lltf0.shape[0], _stream_ptr(stream)))
    return st


def freq_comp11n(in0, in1, first, nbursts, state, stream=None):
    """in0/in1: int16 CUDA [N,2]; first/nbursts: int32 CUDA [nframes]; state: int16 CUDA [nframes,24] (updated in place) -> (out0, out1)."""
    import torch
    o0 = in0.clone(); o1 = in1.clone()
    mx = int(nbursts.max().item()) if nbursts.numel() else 0
    _check(load().sora_hip_freq_comp11n(_dev_ptr(in0), _dev_ptr(in1), _dev_ptr(o0), _dev_ptr(o1), _dev_ptr(first), _dev_ptr(nbursts), _dev_ptr(state),
                                        state.shape[0], mx, _stream_ptr(stream)))
    return o0, o1


def pilot_track11n(x0, x1, first, nsym, state, want_theta=True, stream=None):
    """x0/x1: int16 CUDA [nsym_total,64,2]; first/nsym: int32 CUDA [nframes]; state updated in place -> theta int16 [nsym_total,8] or None."""
    import torch
    th = torch.zeros((x0.shape[0], 8), dtype=torch.int16, device=x0.device) if want_theta else None
    _check(load().sora_hip_pilot_track11n(_dev_ptr(x0), _dev_ptr(x1), _dev_ptr(first), _dev_ptr(nsym), _dev_ptr(state),
                                          _dev_ptr(th) if want_theta else None, state.shape[0], _stream_ptr(stream)))
    return th


def mimo_est11n(ltf0, ltf1, stream=None):
    """ltf0/ltf1: int16 CUDA tensors [n,128,2] (the two HT-LTF symbols of RX chain 0 / 1 after the FFT) -> (h, hinv) int16 [n,2,128,2]."""
    import torch
    n = ltf0.shape[0]
    h = torch.empty((n, 2, 128, 2), dtype=torch.int16, device=ltf0.device); hinv = torch.empty_like(h)
    _check(load().sora_hip_mimo_est11n(_dev_ptr(ltf0), _dev_ptr(ltf1), _dev_ptr(h), _dev_ptr(hinv), n, _stream_ptr(stream)))
    return h, hinv


def mimo_comp11n(hinv, y0, y1, frame_index=None, stream=None):
    """hinv: int16 [nframes,2,128,2]; y0/y1: int16 [nsym,64,2] (RX chain 0 / 1 after the FFT); frame_index: int32/uint32 [nsym] or None
    -> (x0, x1) int16 [nsym,64,2], the two spatial streams."""
    import torch
    x0 = torch.empty_like(y0); x1 = torch.empty_like(y1)
    _check(load().sora_hip_mimo_comp11n(_dev_ptr(hinv), _dev_ptr(frame_index) if frame_index is not None else None, _dev_ptr(y0), _dev_ptr(y1),
                                        _dev_ptr(x0), _dev_ptr(x1), y0.shape[0], _stream_ptr(stream)))
    return x0, x1


def siso_est11n(lltf0, lltf1, stream=None):
    """lltf0/lltf1: int16 CUDA tensors [n,128,2] (the two L-LTF symbols of RX chain 0 / 1 after the FFT) -> ch int16 [n,2,64,2]."""
    import torch
    n = lltf0.shape[0]
    ch = torch.empty((n, 2, 64, 2), dtype=torch.int16, device=lltf0.device)
    _check(load().sora_hip_siso_est11n(_dev_ptr(lltf0), _dev_ptr(lltf1), _dev_ptr(ch), n, _stream_ptr(stream)))
    return ch


def siso_comp11n(ch, y0, y1, frame_index=None, stream=None):
    """ch: int16 [nframes,2,64,2]; y0/y1: int16 [nsym,64,2] -> (x0, x1, mrc) int16 [nsym,64,2] (TSisoChannelComp then TMrcCombine)."""
    import torch
    x0 = torch.empty_like(y0); x1 = torch.empty_like(y1); m = torch.empty_like(y0)
    _check(load().sora_hip_siso_comp11n(_dev_ptr(ch), _dev_ptr(frame_index) if frame_index is not None else None, _dev_ptr(y0), _dev_ptr(y1),
                                        _dev_ptr(x0), _dev_ptr(x1), _dev_ptr(m), y0.shape[0], _stream_ptr(stream)))
    return x0, x1, m


def sig_demap11n(sym, stream=None):
    """sym: int16 [n,3,64,2] (L-SIG, HT-SIG1, HT-SIG2 after MRC) -> soft uint8 [n,144]."""
    import torch
    soft = torch.empty((sym.shape[0], 144), dtype=torch.uint8, device=sym.device)
    _check(load().sora_hip_sig_demap11n(_dev_ptr(sym), _dev_ptr(soft), sym.shape[0], _stream_ptr(stream)))
    return soft


def sig_decode11n(soft, stream=None):
    """soft: uint8 [n,144] (sig_demap11n's output) -> int32 [n,12]: error_code, data_rate_kbps, frame_length, ht_frame_mcs, ht_frame_length,
    code_rate, total_symbols, remain_symbols, symbol_type, L-SIG, HT-SIG bits 0..31, HT-SIG bits 32..41."""
    import torch
    rec = torch.empty((soft.shape[0], 12), dtype=torch.int32, device=soft.device)
    _check(load().sora_hip_sig_decode11n(_dev_ptr(soft), _dev_ptr(rec), soft.shape[0], _stream_ptr(stream)))
    return rec


def deinterleave11a(s, n_bpsc, stream=None):
    import torch
    out = torch.empty_like(s)
    _check(load().sora_hip_deinterleave11a(_dev_ptr(s), _dev_ptr(out), n_bpsc, s.shape[0], _stream_ptr(stream)))
    return out


def viterbi11a(soft, soft_off, nsoft, frame_len, code_rate, out_stride=2560, stream=None):
    """soft: uint8 CUDA tensor; soft_off/nsoft: int32 CUDA tensors [n]; frame_len: int16 CUDA [n]."""
    import torch
    n = soft_off.shape[0]
    out = torch.zeros((n, out_stride), dtype=torch.uint8, device=soft.device)
    out_off = (torch.arange(n, device=soft.device, dtype=torch.int32) * out_stride).contiguous()
    _check(load().sora_hip_viterbi11a(_dev_ptr(soft), _dev_ptr(soft_off), _dev_ptr(nsoft), _dev_ptr(frame_len), code_rate,
                                      _dev_ptr(out), _dev_ptr(out_off), n, _stream_ptr(stream)))
    return out


def viterbi11a_workspace_bytes(soft_span_bytes, n):
    return int(load().sora_hip_viterbi11a_workspace_bytes(int(soft_span_bytes), int(n)))


def viterbi11a_ws(soft, soft_off, nsoft, frame_len, code_rate, workspace, out=None, out_off=None, out_stride=2560, lanes_per_pair=0, stream=None):
    """The Viterbi brick out of a caller-owned workspace (uint8 CUDA tensor of >= viterbi11a_workspace_bytes(soft.numel(), n)):
    no allocation and no host wait inside the call; the caller synchronises the stream before reading `out`.
    lanes_per_pair: 64 (or 0) = k_viterbi, 16 = k_viterbi16, TRELLIS_WINDOWED = k_viterbi16w + k_win_redo."""
    import torch
    n = soft_off.shape[0]
    if out is None:
        out = torch.zeros((n, out_stride), dtype=torch.uint8, device=soft.device)
        out_off = (torch.arange(n, device=soft.device, dtype=torch.int32) * out_stride).contiguous()
    _check(load().sora_hip_viterbi11a_ws(_dev_ptr(soft), soft.numel(), _dev_ptr(soft_off), _dev_ptr(nsoft), _dev_ptr(frame_len), code_rate,
                                         _dev_ptr(out), _dev_ptr(out_off), n, _dev_ptr(workspace), workspace.numel(), int(lanes_per_pair), _stream_ptr(stream)))
    return out


def viterbi11n_workspace_bytes(soft_span_bytes, n):
    return int(load().sora_hip_viterbi11n_workspace_bytes(int(soft_span_bytes), int(n)))


def viterbi11n_ws(soft, soft_off, nsoft, frame_len, code_rate, workspace, out=None, out_off=None, out_stride=2560, lanes_per_pair=0, stream=None):
    """viterbi11a_ws for the 802.11n graph's decoder T11aViterbi<..,192,36>: one byte per soft value (its low three bits), a workspace of
    >= viterbi11n_workspace_bytes(soft.numel(), n).  lanes_per_pair: 64 (or 0), 16 or TRELLIS_WINDOWED."""
    import torch
    n = soft_off.shape[0]
    if out is None:
        out = torch.zeros((n, out_stride), dtype=torch.uint8, device=soft.device)
        out_off = (torch.arange(n, device=soft.device, dtype=torch.int32) * out_stride).contiguous()
    _check(load().sora_hip_viterbi11n_ws(_dev_ptr(soft), soft.numel(), _dev_ptr(soft_off), _dev_ptr(nsoft), _dev_ptr(frame_len), code_rate,
                                         _dev_ptr(out), _dev_ptr(out_off), n, _dev_ptr(workspace), workspace.numel(), int(lanes_per_pair), _stream_ptr(stream)))
    return out


CR_56 = 3


def viterbi56_11n(soft, soft_off, nsoft, frame_len, out=None, out_off=None, out_stride=2560, stream=None):
    """The K=7 decoder at code rate 5/6 (SORA_CR_56: A1 B1 A2 B3 A4 B5) with the 802.11n graph's 192 / 36 window schedule, k_viterbi56_11n: soft = uint8 CUDA
    tensor, one byte per soft value (its low three bits), job i = nsoft[i] bytes at soft_off[i] (uint32 / int32 CUDA tensors), frame_len int16 / uint16.  Nothing at or
    behind soft.numel() is read; no workspace, no allocation beyond `out`, no host wait.  -> out (uint8 [n, out_stride], or the caller's with its out_off)."""
    import torch
    n = soft_off.shape[0]
    if out is None:
        out = torch.zeros((n, out_stride), dtype=torch.uint8, device=soft.device)
        out_off = (torch.arange(n, device=soft.device, dtype=torch.int32) * out_stride).contiguous()
    _check(load().sora_hip_viterbi56_11n(_dev_ptr(soft), soft.numel(), _dev_ptr(soft_off), _dev_ptr(nsoft), _dev_ptr(frame_len), _dev_ptr(out), _dev_ptr(out_off), n,
                                         _stream_ptr(stream)))
    return out


def viterbi_window_stats(workspace, stream=None):
    """The proof record of the last TRELLIS_WINDOWED call of viterbi11a_ws / viterbi11n_ws on `workspace` (waits for `stream`):
    (boundaries, boundaries failed, jobs decoded again, units)."""
    v = (ctypes.c_ulonglong * 4)()
    _check(load().sora_hip_viterbi_window_stats(_dev_ptr(workspace), v, _stream_ptr(stream)))
    return tuple(int(x) for x in v)


INGEST_RXBLOCK, INGEST_RAW14, INGEST_44TO40, INGEST_DECIMATE2 = 1, 2, 4, 8


def ingest_count(raw_bytes, flags):
    return int(load().sora_hip_ingest_count(int(raw_bytes), int(flags)))


def ingest(raw, flags, stream=None, sync=True):
    """raw: uint8 (dump bytes) or int16 [n,2] CUDA tensor -> int16 [m,2] CUDA tensor (de-framed / sign-fixed / 44->40 / decimated).
    sync: wait for the kernel, so that the result can go straight to Rx.process_dev (whose streams do not follow the null stream)."""
    import torch
    nbytes = raw.numel() * raw.element_size()
    n = ingest_count(nbytes, flags)
    out = torch.empty((max(n, 1), 2), dtype=torch.int16, device=raw.device)
    got = ctypes.c_size_t(0)
    _check(load().sora_hip_ingest(_dev_ptr(raw), nbytes, int(flags), _dev_ptr(out), n, ctypes.byref(got), _stream_ptr(stream)))
    if sync:
        _check(load().sora_hip_stream_synchronize(_stream_ptr(stream)))
    return out[:got.value]


def _tx11a_entry(sample_rate_mhz):
    """(samples, call) of the 802.11a transmitter at 40 MHz (`demod11 -m`'s file format) or 44 MHz (a Sora radio's own rate)."""
    if sample_rate_mhz == 40:
        return load().sora_hip_tx11a_samples, load().sora_hip_tx11a
    if sample_rate_mhz == 44:
        return load().sora_hip_tx11a44_samples, load().sora_hip_tx11a44
    raise ValueError("tx11a: sample_rate_mhz must be 40 or 44, not %r" % (sample_rate_mhz,))


def tx11a_samples(mpdu_len_nofcs, rate_kbps, sample_rate_mhz=40):
    """Samples of one 802.11a frame at 40 or 44 MHz (sora_hip_tx11a_samples / sora_hip_tx11a44_samples); 0 for an unsupported rate or length."""
    return int(_tx11a_entry(sample_rate_mhz)[0](int(mpdu_len_nofcs), int(rate_kbps)))


def tx11a(mpdus, rates_kbps, seeds=None, device=0, stream=None, sync=True, gaps=None, sample_rate_mhz=40):
    """Modulate a batch of MPDUs (bytes WITHOUT FCS) on the GPU.  -> (int8 CUDA tensor [total,2] COMPLEX8 @40 MHz, offsets list).
    Frame f occupies samples offsets[f] .. offsets[f+1] (gaps[f] zero samples in front of frame f, if given, included at its start).
    sample_rate_mhz=44: the reference's 44 MHz graphs (TUpsample40MTo44M in front of the pack), samples, offsets and gaps at 44 MHz."""
    import torch
    count, call = _tx11a_entry(sample_rate_mhz)
    n = len(mpdus)
    seeds = [0xFF] * n if seeds is None else list(seeds)
    lens = [len(m) for m in mpdus]
    off = np.zeros(n + 1, np.int64); np.cumsum([(l + 3) // 4 * 4 for l in lens], out=off[1:])
    blob = np.zeros(max(int(off[-1]), 4), np.uint8)
    for f, m in enumerate(mpdus):
        blob[off[f]:off[f] + lens[f]] = np.frombuffer(bytes(m), np.uint8)
    ns = [int(count(int(l), int(r))) for l, r in zip(lens, rates_kbps)]
    if any(v == 0 for v in ns):
        raise SoraError(-1, "tx11a: unsupported rate or length")
    gaps = [0] * n if gaps is None else [int(v) for v in gaps]
    ooff = np.zeros(n + 1, np.uint64); np.cumsum([a + b for a, b in zip(ns, gaps)], out=ooff[1:])
    first = ooff[:-1] + np.asarray(gaps, np.uint64)
    dev = torch.device("cuda", device)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    d_blob = t(blob, np.uint8); d_off = torch.from_numpy(off[:-1].astype(np.int32)).to(dev)
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).to(dev); d_rate = torch.from_numpy(np.asarray(rates_kbps, np.int32)).to(dev)
    d_seed = t(np.asarray(seeds, np.uint8), np.uint8); d_ooff = torch.from_numpy(first.astype(np.int64)).to(dev)
    out = torch.zeros((int(ooff[-1]), 2), dtype=torch.int8, device=dev)
    _check(call(_dev_ptr(d_blob), _dev_ptr(d_off), _dev_ptr(d_len), _dev_ptr(d_rate), _dev_ptr(d_seed), n,
                _dev_ptr(out), _dev_ptr(d_ooff), _stream_ptr(stream)))
    if sync:
        _check(load().sora_hip_stream_synchronize(_stream_ptr(stream)))
    return out, [int(v) for v in ooff]


# ---- the 802.11a modulation graph's bricks as stages (include/sora_hip.h; the byte formats are the bricks': bits packed in bytes, LSB first)
CR_12, CR_23, CR_34 = 0, 1, 2


def _opt_ptr(x):
    return None if x is None else _dev_ptr(x)


def scramble11a(x, off, length, seed, tail=None, max_len=None, stream=None):
    """T11aSc: x uint8 CUDA [nbytes]; off / length (/ tail) int32 CUDA [n]; seed uint8 CUDA [n] -> uint8 CUDA like x (bytes outside every frame are copied).
    tail[f] < length[f]: that byte is TAIL_SCRAMBLE.  max_len: a bound on the lengths (default: read back from `length`)."""
    out = x.clone()
    n = off.shape[0]
    if max_len is None:
        max_len = int(length.max().item()) if n else 0
    _check(load().sora_hip_scramble11a(_dev_ptr(x), _dev_ptr(out), _dev_ptr(off), _dev_ptr(length), _opt_ptr(tail), _dev_ptr(seed), n, int(max_len), _stream_ptr(stream)))
    return out


def conv_encode11a(x, in_off, length, code_rate, out, out_off, max_len=None, stream=None):
    """TConvEncode_12 / _23 / _34 (code_rate = CR_12 / CR_23 / CR_34): frame f reads length[f] bytes at x[in_off[f]:] and writes its whole bursts' 2 / 3 / 4 bytes per
    1 / 2 / 3 into out[out_off[f]:] (uint8 CUDA, written in place and returned); nothing else of `out` is touched."""
    n = in_off.shape[0]
    if max_len is None:
        max_len = int(length.max().item()) if n else 0
    _check(load().sora_hip_conv_encode11a(_dev_ptr(x), _dev_ptr(in_off), _dev_ptr(length), int(code_rate), _dev_ptr(out), _dev_ptr(out_off), n, int(max_len),
                                          _stream_ptr(stream)))
    return out


def interleave11a(s, n_bpsc, stream=None):
    """T11aInterleave*: s uint8 CUDA [n, 6 n_bpsc] -> same shape."""
    import torch
    out = torch.empty_like(s)
    _check(load().sora_hip_interleave11a(_dev_ptr(s), _dev_ptr(out), int(n_bpsc), s.shape[0], _stream_ptr(stream)))
    return out


def map11a(s, n_bpsc, mod=0, stream=None):
    """TMap11a*<MOD>: s uint8 CUDA [n, 6 n_bpsc] -> int16 CUDA [n, 48, 2]; mod = 0: the 802.11a amplitude of n_bpsc."""
    import torch
    out = torch.empty((s.shape[0], 48, 2), dtype=torch.int16, device=s.device)
    _check(load().sora_hip_map11a(_dev_ptr(s), _dev_ptr(out), int(n_bpsc), int(mod), s.shape[0], _stream_ptr(stream)))
    return out


def add_pilot11a(x, first, nsym, bpsk_mod=0, pos0=None, stream=None):
    """T11aAddPilot: x int16 CUDA [n, 48, 2]; first / nsym int32 CUDA [nframes] (pos0: the position in its frame of each entry's first symbol, default 0)
    -> int16 CUDA [n, 64, 2]; symbols no frame owns stay 0."""
    import torch
    out = torch.zeros((x.shape[0], 64, 2), dtype=torch.int16, device=x.device)
    if pos0 is None:
        _check(load().sora_hip_add_pilot11a(_dev_ptr(x), _dev_ptr(out), _dev_ptr(first), _dev_ptr(nsym), first.shape[0], int(bpsk_mod), _stream_ptr(stream)))
    else:
        _check(load().sora_hip_add_pilot11a_from(_dev_ptr(x), _dev_ptr(out), _dev_ptr(first), _dev_ptr(nsym), _dev_ptr(pos0), first.shape[0], int(bpsk_mod),
                                                 _stream_ptr(stream)))
    return out


def ifftx11a(x, stream=None):
    """TIFFTx: x int16 CUDA [n, 64, 2] -> int16 CUDA [n, 160, 2]."""
    import torch
    out = torch.empty((x.shape[0], 160, 2), dtype=torch.int16, device=x.device)
    _check(load().sora_hip_ifftx11a(_dev_ptr(x), _dev_ptr(out), x.shape[0], _stream_ptr(stream)))
    return out


def upsample40to44(x, sees_next=None, stream=None):
    """TUpsample40MTo44M: x int16 CUDA [n, 160, 2] -> int16 CUDA [n, 176, 2]; sees_next uint8 CUDA [n]: block b finds block b + 1's first sample behind its last."""
    import torch
    out = torch.empty((x.shape[0], 176, 2), dtype=torch.int16, device=x.device)
    _check(load().sora_hip_upsample40to44(_dev_ptr(x), _dev_ptr(out), _opt_ptr(sees_next), x.shape[0], _stream_ptr(stream)))
    return out


def pack16to8(x, stream=None):
    """TPackSample16to8: x int16 CUDA [..., 2] of a multiple of 8 samples -> int8 CUDA of the same shape."""
    import torch
    out = torch.empty(x.shape, dtype=torch.int8, device=x.device)
    _check(load().sora_hip_pack16to8(_dev_ptr(x), _dev_ptr(out), x.numel() // 2, _stream_ptr(stream)))
    return out


def preamble11a(ncopies=1, device=0, stream=None):
    """TTS11aSrc: -> int16 CUDA [ncopies, 640, 2], the 802.11a preamble at 40 MHz."""
    import torch
    out = torch.empty((int(ncopies), 640, 2), dtype=torch.int16, device=torch.device("cuda", device))
    _check(load().sora_hip_preamble11a(_dev_ptr(out), int(ncopies), _stream_ptr(stream)))
    return out


_RATES_11A = {6000: (1, CR_12, 24, 0xB), 9000: (1, CR_34, 36, 0xF), 12000: (2, CR_12, 48, 0xA), 18000: (2, CR_34, 72, 0xE),
              24000: (4, CR_12, 96, 0x9), 36000: (4, CR_34, 144, 0xD), 48000: (6, CR_23, 192, 0x8), 54000: (6, CR_34, 216, 0xC)}


def mod11a_fields(mpdu, rate_kbps):
    """What TBB11aSrc::Process (PHY_11a.hpp:111-202) sends down the graph for one MPDU without FCS: (the 3 SIGNAL bytes, which go unscrambled through the 6 Mbps
    path; SERVICE + MPDU + FCS + tail + pad, whole symbols -- two at 9 Mbps; the index of the tail byte)."""
    import zlib
    nb, cr, nd, rc = _RATES_11A[int(rate_kbps)]
    mpdu = bytes(mpdu)
    sig = rc | ((len(mpdu) + 4) << 5)
    sig |= (bin(sig).count("1") & 1) << 17
    ndp = nd * 2 if int(rate_kbps) == 9000 else nd
    dbytes = 2 + len(mpdu) + 4 + 1
    rem = (dbytes * 8) % ndp
    nbytes = dbytes + ((ndp - rem if rem else 0) + 7) // 8
    data = np.zeros(nbytes, np.uint8)
    data[2:2 + len(mpdu)] = np.frombuffer(mpdu, np.uint8)
    data[2 + len(mpdu):2 + len(mpdu) + 4] = np.frombuffer(int(zlib.crc32(mpdu) & 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)
    return np.array([sig & 255, (sig >> 8) & 255, (sig >> 16) & 255], np.uint8), data, dbytes - 1


class Mod11aStages:
    """sora_amd.tx11a's frames composed from the nine stage entry points instead of the fused kernel: CreatePreamble11a_* and CreateModGraph11a_* (fb11amod_config.hpp:74-110)
    brick by brick.  The constructor plays TBB11aSrc on the host (mod11a_fields) and uploads the fields and the frame tables; run() is the stage chain, every
    intermediate through HBM.  The symbols are laid out by modulation (all SIGNAL symbols, then the data symbols of the BPSK, QPSK, 16-QAM and 64-QAM frames), so that
    each stage is ONE call per modulation or code rate whatever the batch; a last index_select puts the 160 / 176-sample blocks into frame order."""

    def __init__(self, mpdus, rates, seeds=None, sample_rate_mhz=40, device=0):
        import torch
        if sample_rate_mhz not in (40, 44):
            raise ValueError("mod11a_by_stages: sample_rate_mhz must be 40 or 44, not %r" % (sample_rate_mhz,))
        n = self.n = len(mpdus)
        self.mhz = sample_rate_mhz
        seeds = [0xFF] * n if seeds is None else list(seeds)
        if any(int(r) not in _RATES_11A or len(m) + 4 > 4095 for m, r in zip(mpdus, rates)):
            raise SoraError(-1, "mod11a_by_stages: unsupported rate or length")
        dev = self.dev = torch.device("cuda", device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        i32 = lambda a: up(np.asarray(a, np.int64).astype(np.int32), np.int32)
        fields = [mod11a_fields(m, r) for m, r in zip(mpdus, rates)]
        par = [_RATES_11A[int(r)] for r in rates]
        nsym = [len(fl[1]) * 8 // p[2] for fl, p in zip(fields, par)]
        # symbol slots: SIGNAL symbols 0 .. n - 1, then the data symbols, frames grouped by modulation (the BPSK group follows the SIGNAL symbols: one BPSK run)
        order = sorted(range(n), key=lambda f: (par[f][0], f))
        slot0 = [0] * n
        at = n
        for f in order:
            slot0[f] = at; at += nsym[f]
        self.nslots = at
        self.run_of = {}                                                         # n_bpsc -> (first slot, slots)
        for nb in (1, 2, 4, 6):
            fs = [f for f in order if par[f][0] == nb]
            cnt = sum(nsym[f] for f in fs)
            self.run_of[nb] = (0, n + cnt) if nb == 1 else (slot0[fs[0]] if fs else at, cnt)
        # the coded bytes of a run lie together, 6 n_bpsc per slot, every run from a 16-byte boundary
        self.cbase, cat = {}, 0
        for nb in (1, 2, 4, 6):
            self.cbase[nb] = cat; cat += (self.run_of[nb][1] * 6 * nb + 15) // 16 * 16
        self.coded_bytes = max(cat, 16)
        coded_off = lambda nb, slot: self.cbase[nb] + (slot - self.run_of[nb][0]) * 6 * nb
        # the uncoded bytes: SIGNAL fields (3 bytes each), then the data fields
        dlen = [len(fl[1]) for fl in fields]
        doff = np.zeros(n + 1, np.int64); np.cumsum(dlen, out=doff[1:]); doff += 3 * n
        raw = np.zeros(max(int(doff[-1]), 1), np.uint8)
        for f, fl in enumerate(fields):
            raw[3 * f:3 * f + 3] = fl[0]; raw[doff[f]:doff[f + 1]] = fl[1]
        self.d_raw = up(raw, np.uint8)
        self.scr = (i32(doff[:-1]), i32(dlen), i32([fl[2] for fl in fields]), up(np.asarray(seeds, np.uint8), np.uint8), max(dlen))
        # TConvEncode_*: the SIGNAL fields at rate 1/2, the data fields by code rate (a fresh register per field)
        self.enc = [(CR_12, i32([3 * f for f in range(n)]), i32([3] * n), i32([coded_off(1, f) for f in range(n)]), n, 3)]
        for cr in (CR_12, CR_23, CR_34):
            fs = [f for f in range(n) if par[f][1] == cr]
            if fs:
                self.enc.append((cr, i32([doff[f] for f in fs]), i32([dlen[f] for f in fs]), i32([coded_off(par[f][0], slot0[f]) for f in fs]), len(fs),
                                 max(dlen[f] for f in fs)))
        # T11aAddPilot: the SIGNAL symbol is position 0 of its frame, the data symbols follow from position 1
        self.pil = (i32(list(range(n)) + slot0), i32([1] * n + nsym), i32([0] * n + [1] * n))
        sees = np.zeros(4 * n + self.nslots, np.uint8); sees[:4 * n] = np.tile([1, 1, 1, 0], n)     # the preamble is one burst: its blocks 0..2 see the next block
        self.d_sees = up(sees, np.uint8)
        blocks = []                                                              # frame order: preamble, SIGNAL, data
        for f in range(n):
            blocks += [4 * f, 4 * f + 1, 4 * f + 2, 4 * f + 3, 4 * n + f] + list(range(4 * n + slot0[f], 4 * n + slot0[f] + nsym[f]))
        self.d_blocks = up(np.asarray(blocks, np.int64), np.int64)
        per = 160 if sample_rate_mhz == 40 else 176
        offs = np.zeros(n + 1, np.int64); np.cumsum([(5 + k) * per for k in nsym], out=offs[1:])
        self.offsets = [int(v) for v in offs]

    def run(self):
        """-> int8 CUDA [total, 2]; everything in order on torch's current stream (the gather at the end is torch's), nothing waited for"""
        import torch
        L = load()
        stream = None
        st = _stream_ptr(stream)
        n, dev, nslots = self.n, self.dev, self.nslots
        off, ln, tail, seed, mx = self.scr
        d_scr = scramble11a(self.d_raw, off, ln, seed, tail=tail, max_len=mx, stream=stream)        # (the SIGNAL bytes pass with NO_SCRAMBLE: in no frame of the call)
        d_coded = torch.empty(self.coded_bytes, dtype=torch.uint8, device=dev)
        for cr, in_off, ilen, out_off, cnt, mx in self.enc:
            _check(L.sora_hip_conv_encode11a(_dev_ptr(d_scr), _dev_ptr(in_off), _dev_ptr(ilen), cr, _dev_ptr(d_coded), _dev_ptr(out_off), cnt, mx, st))
        d_inter = torch.empty_like(d_coded)
        d_car = torch.empty((nslots, 48, 2), dtype=torch.int16, device=dev)
        for nb in (1, 2, 4, 6):                                                  # T11aInterleave* -> TMap11a*, one call per modulation
            s0, ns = self.run_of[nb]
            if ns:
                _check(L.sora_hip_interleave11a(d_coded.data_ptr() + self.cbase[nb], d_inter.data_ptr() + self.cbase[nb], nb, ns, st))
                _check(L.sora_hip_map11a(d_inter.data_ptr() + self.cbase[nb], d_car.data_ptr() + s0 * 192, nb, 0, ns, st))
        d_bins = torch.empty((nslots, 64, 2), dtype=torch.int16, device=dev)     # (every slot belongs to a frame)
        _check(L.sora_hip_add_pilot11a_from(_dev_ptr(d_car), _dev_ptr(d_bins), _dev_ptr(self.pil[0]), _dev_ptr(self.pil[1]), _dev_ptr(self.pil[2]), 2 * n, 0, st))
        # TTS11aSrc and TIFFTx into one 16-bit stream of 160-sample blocks: n preambles (4 blocks each), then the symbol slots
        d_x = torch.empty((4 * n + nslots, 160, 2), dtype=torch.int16, device=dev)
        _check(L.sora_hip_preamble11a(d_x.data_ptr(), n, st))
        _check(L.sora_hip_ifftx11a(d_bins.data_ptr(), d_x.data_ptr() + 4 * n * 640, nslots, st))
        if self.mhz == 44:
            d_x = upsample40to44(d_x, self.d_sees, stream=stream)
        return pack16to8(d_x, stream=stream).index_select(0, self.d_blocks).reshape(-1, 2)


def mod11a_by_stages(mpdus, rates, seeds=None, sample_rate_mhz=40, device=0, sync=True):
    """Modulate a batch of MPDUs (bytes WITHOUT FCS) through the stage chain (Mod11aStages) -> (int8 CUDA [total, 2], offsets): the same as sora_amd.tx11a returns."""
    plan = Mod11aStages(mpdus, rates, seeds, sample_rate_mhz, device)
    out = plan.run()
    if sync:
        _check(load().sora_hip_stream_synchronize(_stream_ptr(None)))
    return out, plan.offsets


# ---- the 802.11b receive graph's bricks as stages (include/sora_hip.h: sora_hip_*11b) -----------------------------
# Records, as int32 words per stream (a complex16 is one word: re | im << 16):
#   stream state [n, 4]   last_symbol, byte_reg, is_even, reserved                         (sora_stream11b_state)
#   energy       [n, 17]  average_energy, window[8], idx, count, power_detected, error_code, cca_pwr_threshold, update_cnt, sum_dc, dc
#   symtiming    [n, 2]   m_index, m_frag
#   barker       [n, 15]  sync_flag, last_peak_cnt, m_max, search_count, partial[10], error_code
#   sfd          [n, 9]   last_symbol, byte_reg, bit_one_found, bit_zero_found, word, bit_err_cnt, sync_cnt, rxrate_state, error_code
STATE11B_WORDS = {"stream": 4, "energy": 17, "symtiming": 2, "barker": 15, "sfd": 9, "plcp": 4, "sink": 2}
RATE11B_SYNC, RATE11B_1M, RATE11B_2M, RATE11B_5P5M, RATE11B_11M = range(5)


def state11b_reset(kind, n, cca_pwr_threshold=1000 * 1000):
    """-> int32 numpy [n, words]: the record `kind` of STATE11B_WORDS as the brick holds it after Reset in a fresh context (every context field 0)"""
    s = np.zeros((n, STATE11B_WORDS[kind]), np.int32)
    if kind == "energy":
        s[:, 13] = cca_pwr_threshold; s[:, 14] = 8
    elif kind == "symtiming":
        s[:, 0] = 2
    elif kind == "barker":
        s[:, 1] = -1
    return s


def _max_n(n, max_n):
    return int(n.max().item()) if max_n is None and n.shape[0] else int(max_n or 0)


def dc_remove11b(x, first, n, out_first, dc, out, max_n=None, stream=None):
    """TDCRemove: x / out int16 CUDA [samples, 2]; first / n / out_first int32 CUDA [streams] (n in bursts of 4 samples, the offsets in samples); dc int16 CUDA
    [streams, 2] -> out, stream f's 4 n[f] samples from out_first[f] written in place"""
    _check(load().sora_hip_dc_remove11b(_dev_ptr(x), _dev_ptr(first), _dev_ptr(n), _dev_ptr(out_first), _dev_ptr(dc), _dev_ptr(out), first.shape[0], _max_n(n, max_n),
                                        _stream_ptr(stream)))
    return out


def _search11b(fn, x, first, n, state, max_n, stream, *extra):
    import torch
    used = torch.zeros(first.shape[0], dtype=torch.int32, device=x.device)
    _check(getattr(load(), fn)(_dev_ptr(x), _dev_ptr(first), _dev_ptr(n), _dev_ptr(state), _dev_ptr(used), first.shape[0], _max_n(n, max_n), *extra, _stream_ptr(stream)))
    return used


def energy_detect11b(x, first, n, state, max_n=None, stream=None):
    """TEnergyDetect + TDCEstimator: x = DC-removed samples; n in bursts of 4; state int32 CUDA [streams, 17] (in / out) -> used int32 CUDA [streams]: the bursts consumed"""
    return _search11b("sora_hip_energy_detect11b", x, first, n, state, max_n, stream)


def barker_sync11b(x, first, n, state, max_n=None, stream=None):
    """TBarkerSync: x = chips; n in chips; state int32 CUDA [streams, 15] (in / out) -> used: the chips swallowed"""
    return _search11b("sora_hip_barker_sync11b", x, first, n, state, max_n, stream)


def sfd_sync11b(x, first, n, state, mode=0, max_n=None, stream=None):
    """TSFDSync (mode 1: with the short preamble): x = symbols; n in symbols; state int32 CUDA [streams, 9] (in / out) -> used: the symbols consumed"""
    return _search11b("sora_hip_sfd_sync11b", x, first, n, state, max_n, stream, int(mode))


def symtiming11b(x, first, n, out_first, state, out, max_n=None, stream=None):
    """TSymTiming: n in blocks of 28 samples; state int32 CUDA [streams, 2] (in / out); out int16 CUDA [chips, 2] with room for 8 n[f] chips from out_first[f]
    -> nchips int32 CUDA [streams]: the chips written"""
    import torch
    nchips = torch.zeros(first.shape[0], dtype=torch.int32, device=x.device)
    _check(load().sora_hip_symtiming11b(_dev_ptr(x), _dev_ptr(first), _dev_ptr(n), _dev_ptr(out_first), _dev_ptr(state), _dev_ptr(out), _dev_ptr(nchips), first.shape[0],
                                        _max_n(n, max_n), _stream_ptr(stream)))
    return nchips


def despread11b(x, first, n, out_first, out, max_n=None, stream=None):
    """TBB11bDespread: n[f] symbols from the 11 n[f] chips at chip first[f] -> out (symbols, written from out_first[f])"""
    _check(load().sora_hip_despread11b(_dev_ptr(x), _dev_ptr(first), _dev_ptr(n), _dev_ptr(out_first), _dev_ptr(out), first.shape[0], _max_n(n, max_n), _stream_ptr(stream)))
    return out


def _stream11b(fn, x, first, n, out_first, state, out, max_n, stream):
    _check(getattr(load(), fn)(_dev_ptr(x), _dev_ptr(first), _dev_ptr(n), _dev_ptr(out_first), _dev_ptr(state), _dev_ptr(out), first.shape[0], _max_n(n, max_n),
                               _stream_ptr(stream)))
    return out


def dbpsk_demap11b(x, first, n, out_first, state, out, max_n=None, stream=None):
    """TDBPSKDemap: n[f] bytes from the 8 n[f] symbols at symbol first[f] -> out uint8 CUDA (from byte out_first[f]); state int32 CUDA [streams, 4] (last_symbol in / out)"""
    return _stream11b("sora_hip_dbpsk_demap11b", x, first, n, out_first, state, out, max_n, stream)


def dqpsk_demap11b(x, first, n, out_first, state, out, max_n=None, stream=None):
    """TDQPSKDemap: n[f] bytes from 4 n[f] symbols (as dbpsk_demap11b)"""
    return _stream11b("sora_hip_dqpsk_demap11b", x, first, n, out_first, state, out, max_n, stream)


def cck5p5_decode11b(x, first, n, out_first, state, out, max_n=None, stream=None):
    """TCCK5P5Decoder: n[f] bytes from 16 n[f] chips; state: last_symbol"""
    return _stream11b("sora_hip_cck5p5_decode11b", x, first, n, out_first, state, out, max_n, stream)


def cck11_decode11b(x, first, n, out_first, state, out, max_n=None, stream=None):
    """TCCK11Decoder: n[f] bytes from 8 n[f] chips; state: last_symbol and is_even"""
    return _stream11b("sora_hip_cck11_decode11b", x, first, n, out_first, state, out, max_n, stream)


def desc741_11b(x, first, n, out_first, state, out, max_n=None, stream=None):
    """TDesc741: n[f] bytes from byte first[f] of x (uint8 CUDA); state: byte_reg"""
    return _stream11b("sora_hip_desc741_11b", x, first, n, out_first, state, out, max_n, stream)


def plcp_parse11b(hdr, stream=None):
    """TBB11bPlcpParser: hdr uint8 CUDA [n, 6] -> int32 CUDA [n, 4]: error_code, data_rate_kbps, frame_length, rxrate_state"""
    import torch
    rec = torch.zeros((hdr.shape[0], 4), dtype=torch.int32, device=hdr.device)
    _check(load().sora_hip_plcp_parse11b(_dev_ptr(hdr), _dev_ptr(rec), hdr.shape[0], _stream_ptr(stream)))
    return rec


def frame_sink11b(x, first, length, stream=None):
    """TBB11bFrameSink: frame f = the descrambled bytes from byte first[f] of x (uint8 CUDA), length[f] = frame_length -> int32 CUDA [n, 2]: error_code, frame_crc32"""
    import torch
    rec = torch.zeros((first.shape[0], 2), dtype=torch.int32, device=x.device)
    _check(load().sora_hip_frame_sink11b(_dev_ptr(x), _dev_ptr(first), _dev_ptr(length), _dev_ptr(rec), first.shape[0], _stream_ptr(stream)))
    return rec


class _Gpu11bOps:
    """rx11b_stages' bricks on the GPU: host tables and records (numpy) up, one stage call, the records and counts back.  Buffers are torch CUDA tensors."""

    def __init__(self, device):
        import torch
        self.torch = torch; self.dev = device

    def _up(self, a, dt=np.int32):
        return self.torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt, copy=False))).to(self.dev)

    def alloc_c16(self, n):
        return self.torch.zeros((max(int(n), 1), 2), dtype=self.torch.int16, device=self.dev)

    def alloc_u8(self, n):
        return self.torch.zeros(max(int(n), 1), dtype=self.torch.uint8, device=self.dev)

    def host_u8(self, buf, a, b):
        return buf[a:b].cpu().numpy().tobytes()

    def dc_remove(self, x, first, n, out_first, dc, out):
        dc_remove11b(x, self._up(first), self._up(n), self._up(out_first), self._up(dc).view(self.torch.int16).reshape(-1, 2), out, max_n=int(max(n)))

    def _search(self, fn, x, first, n, state, *extra):
        st = self._up(state)
        used = fn(x, self._up(first), self._up(n), st, *extra, max_n=int(max(n)))
        return st.cpu().numpy(), used.cpu().numpy()

    def energy_detect(self, x, first, n, state):
        return self._search(energy_detect11b, x, first, n, state)

    def barker_sync(self, x, first, n, state):
        return self._search(barker_sync11b, x, first, n, state)

    def sfd_sync(self, x, first, n, state, mode):
        return self._search(sfd_sync11b, x, first, n, state, mode)

    def symtiming(self, x, first, n, out_first, state, out):
        st = self._up(state)
        nchips = symtiming11b(x, self._up(first), self._up(n), self._up(out_first), st, out, max_n=int(max(n)))
        return st.cpu().numpy(), nchips.cpu().numpy()

    def despread(self, x, first, n, out_first, out):
        despread11b(x, self._up(first), self._up(n), self._up(out_first), out, max_n=int(max(n)))

    def stream_stage(self, kind, x, first, n, out_first, state, out):
        fn = {"dbpsk": dbpsk_demap11b, "dqpsk": dqpsk_demap11b, "cck5p5": cck5p5_decode11b, "cck11": cck11_decode11b, "desc741": desc741_11b}[kind]
        st = self._up(state)
        fn(x, self._up(first), self._up(n), self._up(out_first), st, out, max_n=int(max(n)))
        return st.cpu().numpy()

    def plcp_parse(self, hdr, nhdr):
        return plcp_parse11b(hdr[:6 * nhdr].reshape(nhdr, 6)).cpu().numpy()

    def frame_sink(self, x, first, length):
        return frame_sink11b(x, self._up(first), self._up(length)).cpu().numpy()


def rx11b_stages(ops, iq, descs, mode=0, cca_pwr_threshold=1000 * 1000):
    """The 802.11b receive graph (CreateDemodGraph under MAC11b_Receive, fb11b_demod.cpp:27-76) up to the FIRST event of every capture, composed from the thirteen brick
    stages through `ops` (the GPU's: rx11b_by_stages; the C model's: tests/rx11b_stage_model.first_event).  The host plays the three routing bricks (TBB11bRxSwitch,
    TBB11bRxRateSel, TBB11bPlcpSwitch) and the harness: it reads every stage's counts and records back and builds the next stage's tables from them.
    iq: the captures' samples (ops' buffer), descs: [(first sample, samples)], whole 28-sample source calls each.
    -> per capture None (carrier sense never fires, or the capture ends first) or a dict error_code, rate_kbps, length, crc32, flags, mpdu."""
    nc = len(descs)
    off = np.array([int(d[0]) for d in descs], np.int64); ns = np.array([int(d[1]) for d in descs], np.int64)
    if nc == 0:
        return []
    if (ns % 28).any() or (off % 4).any():
        raise ValueError("rx11b_stages: a capture is whole 28-sample source calls at an offset of whole bursts")
    u32 = lambda a: np.asarray(a, np.int64).astype(np.uint32).view(np.int32)
    events = [None] * nc
    d_dcr = ops.alloc_c16(int((off + ns).max()))
    # ---- the front: TDCRemove -> TBB11bRxSwitch -> TEnergyDetect -> TDCEstimator, in pieces that end where the estimator changes dc (every eighth burst, the burst that
    # finds update_cnt 0): the bursts of a piece see one dc.  SORA_E_CS_TIMEOUT is the harness's: the rest of the 28-sample source call is dropped, the graph reset.
    nb = ns // 4
    est = state11b_reset("energy", nc, cca_pwr_threshold)
    pos = np.zeros(nc, np.int64)
    active = nb > 0
    while active.any():
        n = np.where(active, np.minimum(est[:, 14].astype(np.int64) + 1, nb - pos), 0)
        first = off + 4 * pos
        ops.dc_remove(iq, u32(first), u32(n), u32(first), est[:, 16], d_dcr)
        est, used = ops.energy_detect(d_dcr, u32(first), u32(n), est)
        est = est.copy(); pos += used.astype(np.int64)
        for c in np.nonzero(active)[0]:
            if est[c, 11]:
                active[c] = False
            elif est[c, 12]:
                pos[c] = (pos[c] + 6) // 7 * 7
                dc = est[c, 16]
                est[c] = state11b_reset("energy", 1, cca_pwr_threshold)[0]; est[c, 16] = dc
            if pos[c] >= nb[c]:
                active[c] = False
    live = [c for c in range(nc) if est[c, 11]]
    if not live:
        return events
    # ---- behind the switch: TDCRemove (dc stands still: the estimator is gated) -> TSymTiming over the rest of the capture, in blocks counted from the first burst routed
    blocks = np.array([(ns[c] - 4 * pos[c]) // 28 for c in live], np.int64)
    first = np.array([off[c] + 4 * pos[c] for c in live], np.int64)
    chip0 = np.concatenate([[0], np.cumsum(8 * blocks)])[:-1]
    d_chips = ops.alloc_c16(int(8 * blocks.sum()) + 16)
    nchips = np.zeros(len(live), np.int64)
    if blocks.max() > 0:
        ops.dc_remove(iq, u32(first), u32(7 * blocks), u32(first), est[live, 16], d_dcr)
        _, nch = ops.symtiming(d_dcr, u32(first), u32(blocks), u32(chip0), state11b_reset("symtiming", len(live)), d_chips)
        nchips = nch.astype(np.int64)
    cc = np.zeros(len(live), np.int64)                                         # chips consumed, per live capture
    short = np.zeros(len(live), bool)

    def event(j, err, kbps=0, length=0, crc=0, mpdu=b""):
        events[live[j]] = {"error_code": int(err) & 0xFFFFFFFF, "rate_kbps": int(kbps), "length": int(length), "crc32": int(crc) & 0xFFFFFFFF,
                           "flags": ROW_SHORT_PREAMBLE if short[j] else 0, "mpdu": mpdu}

    # ---- TBarkerSync
    go = list(range(len(live)))
    bst, used = ops.barker_sync(d_chips, u32(chip0), u32(nchips), state11b_reset("barker", len(live)))
    cc += used.astype(np.int64)
    nxt = []
    for j in go:
        if bst[j, 14]:
            event(j, bst[j, 14])
        elif bst[j, 0] == 4:
            nxt.append(j)
    go = nxt
    if not go:
        return events
    # ---- TBB11bRxRateSel port 0: TBB11bDespread -> TSFDSync (145 symbols decide)
    sym0 = np.concatenate([[0], np.cumsum(nchips // 11 + 16)])[:-1]
    d_sym = ops.alloc_c16(int((nchips // 11 + 16).sum()))
    nsym = np.array([min((nchips[j] - cc[j]) // 11, 160) for j in go], np.int64)
    ops.despread(d_chips, u32(chip0[go] + cc[go]), u32(nsym), u32(sym0[go]), d_sym)
    sst, used = ops.sfd_sync(d_sym, u32(sym0[go]), u32(nsym), state11b_reset("sfd", len(go)), mode)
    sstate = state11b_reset("stream", len(live))                                # CF_DifferentialDemap, CF_Descramber: what TSFDSync leaves is what the demappers find
    rate = np.zeros(len(live), np.int64)
    nxt = []
    for k, j in enumerate(go):
        cc[j] += 11 * int(used[k])
        rate[j] = sst[k, 7]; short[j] = bool(sst[k, 3]) and rate[j] != RATE11B_SYNC
        sstate[j, 0] = sst[k, 0]; sstate[j, 1] = sst[k, 1]
        if sst[k, 8]:
            event(j, sst[k, 8])
        elif rate[j] != RATE11B_SYNC:
            nxt.append(j)
    go = nxt
    # ---- the PLCP header: 48 symbols through TDBPSKDemap (RATE_1M) or 24 through TDQPSKDemap (RATE_2M, behind a short SFD) -> TDesc741 -> TBB11bPlcpParser
    d_raw = ops.alloc_u8(4096 * len(live)); d_bytes = ops.alloc_u8(4096 * len(live)); d_hdr = ops.alloc_u8(6 * len(live))
    byte0 = 4096 * np.arange(len(live), dtype=np.int64)

    def demod(js, r, nbytes, out, out_first):
        """nbytes[k] descrambled bytes of capture js[k] at rate r, from its chip cursor, into out at out_first[k]"""
        js = list(js); nbytes = np.asarray(nbytes, np.int64)
        if r in (RATE11B_1M, RATE11B_2M):
            per = 8 if r == RATE11B_1M else 4
            ops.despread(d_chips, u32(chip0[js] + cc[js]), u32(per * nbytes), u32(sym0[js]), d_sym)
            sstate[js] = ops.stream_stage("dbpsk" if r == RATE11B_1M else "dqpsk", d_sym, u32(sym0[js]), u32(nbytes), u32(byte0[js]), sstate[js], d_raw)
            cc[js] += 11 * per * nbytes
        else:
            per = 16 if r == RATE11B_5P5M else 8
            sstate[js] = ops.stream_stage("cck5p5" if r == RATE11B_5P5M else "cck11", d_chips, u32(chip0[js] + cc[js]), u32(nbytes), u32(byte0[js]), sstate[js], d_raw)
            cc[js] += per * nbytes
        sstate[js] = ops.stream_stage("desc741", d_raw, u32(byte0[js]), u32(nbytes), u32(out_first), sstate[js], out)

    chips_per_byte = {RATE11B_1M: 88, RATE11B_2M: 44, RATE11B_5P5M: 16, RATE11B_11M: 8}
    hdr_of = []                                                                 # captures with a whole header, in d_hdr's order
    for r in (RATE11B_1M, RATE11B_2M):
        js = [j for j in go if rate[j] == r and nchips[j] - cc[j] >= 6 * chips_per_byte[r]]
        if js:
            demod(js, r, [6] * len(js), d_hdr, 6 * (len(hdr_of) + np.arange(len(js), dtype=np.int64)))
            hdr_of += js
    if not hdr_of:
        return events
    rec = ops.plcp_parse(d_hdr, len(hdr_of))
    length = np.zeros(len(live), np.int64); kbps = np.zeros(len(live), np.int64)
    go = []
    for k, j in enumerate(hdr_of):
        if rec[k, 0]:
            event(j, rec[k, 0])
            continue
        kbps[j] = rec[k, 1]; length[j] = rec[k, 2]
        if rec[k, 3]:
            rate[j] = rec[k, 3]
        # an unknown SIGNAL (length 0) and lengths below 4 never let TBB11bFrameSink decide; a frame the capture cuts off raises nothing either (nor, here, one
        # longer than the harness's 4096-byte buffer)
        if kbps[j] and 4 <= length[j] <= 4096 and nchips[j] - cc[j] >= (length[j] - 1) * chips_per_byte[int(rate[j])]:
            go.append(j)
    # ---- the payload: frame_length - 1 bytes (the sink decides one byte early) through the rate's demodulator -> TDesc741 -> TBB11bFrameSink
    for r in (RATE11B_1M, RATE11B_2M, RATE11B_5P5M, RATE11B_11M):
        js = [j for j in go if rate[j] == r]
        if js:
            demod(js, r, length[js] - 1, d_bytes, byte0[js])
    if go:
        rec = ops.frame_sink(d_bytes, u32(byte0[go]), u32(length[go]))
        for k, j in enumerate(go):
            if rec[k, 0]:
                event(j, rec[k, 0], kbps[j], length[j], rec[k, 1], ops.host_u8(d_bytes, int(byte0[j]), int(byte0[j] + length[j] - 1)) + b"\0")
    return events


def rx11b_by_stages(d_iq, descs, mode=0, cca_pwr_threshold=1000 * 1000):
    """The first event of every capture of a batch, through the thirteen 802.11b stage entry points alone (rx11b_stages with the GPU's bricks): d_iq int16 CUDA
    [samples, 2] at 44 MHz, descs [(first sample, samples)], mode as Rx11b.set_preamble -> per capture None or a dict error_code, rate_kbps, length, crc32, flags
    (ROW_SHORT_PREAMBLE), mpdu.  The MPDU's last byte and crc32's top byte are 0: what the reference's sink holds for the first frame of a capture.
    A DEMONSTRATION and a test vehicle, not a fast path: between stages it reads counts and records back to the host to build the next tables, some twenty round trips
    per hundred bursts of silence in front of the frame.  The counterpart of mod11a_by_stages; the fast path is Rx11b."""
    return rx11b_stages(_Gpu11bOps(d_iq.device), d_iq, descs, mode, cca_pwr_threshold)


# ---- the bricks that complete the 802.11n receive graph as stages (include/sora_hip.h, sora_hip_cca11n .. sora_hip_frame_sink11a)
# sora_cca11n_state as int32 words [n, 264]: 0 cca_state, 1 error_code, 2 cca_pwr_reading, 3 sense_count, 4 peak_found, 5 peak_count, 6 his_index, 7 timeouts,
# 8..135 his_moving_energy (low, high) x 64, 136..199 / 200..263 the last 64 samples of chain 0 / 1 (re | im << 16), oldest first
CCA11N_WORDS = 264
CCA11N_REARM = 1


def cca11n_states(n):
    """-> int32 numpy [n, 264]: sora_cca11n_state as a constructed TCCA11n holds it in a fresh context: all 0 but the ring, which is LLONG_MAX"""
    s = np.zeros((n, CCA11N_WORDS), np.int32)
    s[:, 8:136:2] = -1; s[:, 9:136:2] = 0x7FFFFFFF
    return s


def cca11n(in0, in1, first, n, state, flags=0, max_n=None, stream=None):
    """TCCA11n: in0 / in1 int16 CUDA [samples, 2], the two chains at 20 MHz; first (samples) / n (bursts of 4) int32 CUDA [streams]; state int32 CUDA [streams, 264]
    (in / out) -> used int32 CUDA [streams]: the bursts consumed"""
    import torch
    used = torch.zeros(first.shape[0], dtype=torch.int32, device=in0.device)
    _check(load().sora_hip_cca11n(_dev_ptr(in0), _dev_ptr(in1), _dev_ptr(first), _dev_ptr(n), _dev_ptr(state), _dev_ptr(used), first.shape[0], _max_n(n, max_n), int(flags),
                                  _stream_ptr(stream)))
    return used


def data_symbol11n(in0, in1, first, nsym, out_first, out0, out1, max_nsym=None, stream=None):
    """T11nDataSymbol: frame f's nsym[f] symbols of 80 samples from sample first[f] of in0 / in1 -> their samples 16..79 at symbol out_first[f] of out0 / out1 (int16 CUDA
    [symbols * 64, 2])"""
    _check(load().sora_hip_data_symbol11n(_dev_ptr(in0), _dev_ptr(in1), _dev_ptr(first), _dev_ptr(nsym), _dev_ptr(out_first), _dev_ptr(out0), _dev_ptr(out1), first.shape[0],
                                          _max_n(nsym, max_nsym), _stream_ptr(stream)))
    return out0, out1


def stream_join11n(s0, s1, n_bpsc, out=None, stream=None):
    """TStreamJoin + TStreamConcat: s0 / s1 uint8 CUDA [n, 52 n_bpsc] -> uint8 CUDA [n, 104 n_bpsc], groups of max(n_bpsc / 2, 1) bytes alternating stream 0 / 1"""
    import torch
    n = s0.shape[0]
    if out is None:
        out = torch.empty((n, 104 * n_bpsc), dtype=torch.uint8, device=s0.device)
    _check(load().sora_hip_stream_join11n(_dev_ptr(s0), _dev_ptr(s1), _dev_ptr(out), int(n_bpsc), n, _stream_ptr(stream)))
    return out


def desc11a(dec, off, length, out, out_off, stream=None):
    """T11aDesc: frame i = length[i] + 2 decoded bytes at dec[off[i]] (uint8 CUDA) -> length[i] descrambled bytes at out[out_off[i]]"""
    _check(load().sora_hip_desc11a(_dev_ptr(dec), _dev_ptr(off), _dev_ptr(length), _dev_ptr(out), _dev_ptr(out_off), off.shape[0], _stream_ptr(stream)))
    return out


def frame_sink11a(x, off, length, stream=None):
    """TBB11aFrameSink: frame i = length[i] descrambled bytes at x[off[i]] (uint8 CUDA) -> int32 CUDA [n, 2]: error_code, frame_crc32"""
    import torch
    rec = torch.zeros((off.shape[0], 2), dtype=torch.int32, device=x.device)
    _check(load().sora_hip_frame_sink11a(_dev_ptr(x), _dev_ptr(off), _dev_ptr(length), _dev_ptr(rec), off.shape[0], _stream_ptr(stream)))
    return rec


class _Gpu11nOps:
    """rx11n_stages' bricks on the GPU: host tables and records (numpy) up, one stage call, records back.  Buffers are torch CUDA tensors."""

    def __init__(self, device):
        import torch
        self.torch = torch; self.dev = device; self.comp = None

    def _up(self, a, dt=np.int32):
        return self.torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt, copy=False))).to(self.dev)

    def host(self, a):
        return a.cpu().numpy()

    def downsample2(self, iq):
        return ingest(iq, INGEST_DECIMATE2)

    def cca(self, x0, x1, first, n, state, flags):
        st = self._up(state)
        used = cca11n(x0, x1, self._up(first), self._up(n), st, flags, max_n=int(max(n)))
        return st.cpu().numpy(), used.cpu().numpy()

    def take(self, x, starts, length):
        idx = (self._up(starts, np.int64)[:, None] + self.torch.arange(length, device=self.dev)[None, :]).reshape(-1)
        return x[idx].contiguous()

    def rows(self, a, idx):
        return a[self._up(idx, np.int64)].contiguous()

    def concat(self, parts):
        return self.torch.cat([p.reshape(-1) for p in parts]).contiguous()

    def cfo_est(self, l0, l1):
        return cfo_est11n(l0.reshape(-1, 128, 2), l1.reshape(-1, 128, 2))

    def freq_comp(self, x0, x1, first, nbursts, state):
        if self.comp is None:
            self.comp = (self.torch.zeros_like(x0), self.torch.zeros_like(x1))
        d_first, d_n = self._up(first), self._up(nbursts)                           # (held until the call has been issued on the null stream, which orders their reuse)
        _check(load().sora_hip_freq_comp11n(_dev_ptr(x0), _dev_ptr(x1), _dev_ptr(self.comp[0]), _dev_ptr(self.comp[1]), _dev_ptr(d_first), _dev_ptr(d_n),
                                            _dev_ptr(state), state.shape[0], int(max(nbursts)), None))
        return self.comp

    def data_symbol(self, x0, x1, first, nsym, out_first, total):
        o0 = self.torch.zeros((max(total, 1) * 64, 2), dtype=self.torch.int16, device=self.dev); o1 = self.torch.zeros_like(o0)
        data_symbol11n(x0, x1, self._up(first), self._up(nsym), self._up(out_first), o0, o1, max_nsym=int(max(nsym)))
        return o0[:total * 64], o1[:total * 64]

    def fft64(self, x):
        return fft64(x.reshape(-1, 64, 2)).reshape(-1, 2)

    def siso_est(self, l0, l1):
        return siso_est11n(l0.reshape(-1, 128, 2), l1.reshape(-1, 128, 2))

    def siso_comp_mrc(self, ch, y0, y1, frame_index):
        return siso_comp11n(ch, y0.reshape(-1, 64, 2), y1.reshape(-1, 64, 2), self._up(frame_index))[2].reshape(-1, 2)

    def sig_demap(self, mrc):
        return sig_demap11n(mrc.reshape(-1, 3, 64, 2))

    def sig_decode(self, soft):
        return sig_decode11n(soft).cpu().numpy().view(np.uint32)

    def mimo_est(self, l0, l1):
        return mimo_est11n(l0.reshape(-1, 128, 2), l1.reshape(-1, 128, 2))[1]

    def mimo_comp(self, hinv, y0, y1, frame_index):
        a, b = mimo_comp11n(hinv, y0.reshape(-1, 64, 2), y1.reshape(-1, 64, 2), self._up(frame_index))
        return a, b

    def pilot_track(self, x0, x1, first, nsym, state):
        pilot_track11n(x0, x1, self._up(first), self._up(nsym), state, want_theta=False)

    def demap_deint(self, x, nb, iss):
        return deinterleave11n(demap11n(x, nb), nb, iss)

    def stream_join(self, s0, s1, nb):
        return stream_join11n(s0, s1, nb)

    def viterbi(self, soft, soft_off, nsoft, lens, code_rate):
        ws = self.torch.empty(viterbi11n_workspace_bytes(soft.numel(), len(lens)), dtype=self.torch.uint8, device=self.dev)
        out = viterbi11n_ws(soft, self._up(soft_off), self._up(nsoft), self._up(lens, np.int16), int(code_rate), ws)
        self.torch.cuda.synchronize(self.dev)
        return out.reshape(-1)

    def desc(self, dec, off, lens, out_off, total):
        out = self.torch.zeros(max(total, 1), dtype=self.torch.uint8, device=self.dev)
        return desc11a(dec, self._up(off), self._up(lens), out, self._up(out_off))

    def frame_sink(self, x, off, lens):
        return frame_sink11a(x, self._up(off), self._up(lens)).cpu().numpy().view(np.uint32)


def sig_gate11n(rec, mcs_max=10):
    """T11nSigParser's checks in its order (PHY_11n.hpp:432-513) on the decoded bits of one sora_hip_sig_decode11n record (words 9..11), with the gate `mcs >= 11`
    at mcs_max + 1 -> None (SORA_E_PLCP_HEADER_FAIL) or (mcs, ht_length, code_rate, data symbols)"""
    sig = int(rec[9]) & 0xFFFFFF; ht = int(rec[10]) | (int(rec[11]) << 32)
    if (sig & 0xFC0010) or (bin(sig).count("1") & 1) or (sig & 0xF) < 8 or ((sig >> 5) & 0xFFF) * 2 > 1500:
        return None
    crc = 0xFF
    for b in range(34):
        crc ^= (ht >> b) & 1
        crc = (crc >> 1) ^ 0xE0 if crc & 1 else crc >> 1
    if ((~crc) & 0xFF) != ((ht >> 34) & 0x3FFF):
        return None
    mcs = ht & 0x7F; length = (ht >> 8) & 0xFFFF
    if mcs < 8 or mcs > mcs_max or length > 1500:
        return None
    cr = 2 if mcs in (10, 12, 14) else 1 if mcs == 13 else 0
    nd = (52, 104, 156, 208, 312, 416, 468)[mcs - 8]
    return mcs, length, cr, (length * 8 + 22 + nd - 1) // nd


def rx11n_stages(ops, iq0, iq1, descs, mcs_max=10, trace=None):
    """The 802.11n 2x2 receive graph (CreateDemodGraph11n under RxThread, fb11n_demod.cpp:30-85) up to the FIRST event of every capture, composed from the brick stages
    through `ops` (the GPU's: rx11n_by_stages; the model's: tests/rx11n_stage_model.first_events), along the walk of oracle/so_rx11n.c:157-239.  The host plays the routing
    bricks (RxSwitch, T11nSymSel, T11nRxRateSel, Mimo64Join, TStreamFork), the parser's gate at mcs_max and the harness: it reads counts and records back and builds the next
    stage's tables from them.  Each phase is one call over all captures still alive; the data field goes symbol by symbol, because TPilotTrack_11n's phase of symbol k
    steers TFreqComp_11n on symbol k + 1.
    iq0 / iq1: the two chains at 40 MHz (ops' buffers), descs: [(first sample, samples)], whole 28-sample source calls at even offsets.
    -> per capture None (no detection, or the capture ends before the event: the end-of-capture flush of zero-padded symbols is not reproduced) or a dict error_code,
    rate_kbps (= MCS), length, crc32, mpdu.  Carrier-sense time-outs re-arm at the burst that raises them (SORA_CCA11N_REARM); RxThread re-arms at the end of its
    28-sample source call, up to three bursts later.  trace: a list that receives (name, host copy) of what each phase hands on."""
    nc = len(descs)
    if nc == 0:
        return []
    off = np.array([int(d[0]) for d in descs], np.int64); ns = np.array([int(d[1]) for d in descs], np.int64)
    if (ns % 28).any() or (off % 2).any():
        raise ValueError("rx11n_stages: a capture is whole 28-sample source calls at an even offset")
    u32 = lambda a: np.asarray(a, np.int64).astype(np.uint32).view(np.int32)

    def note(name, a, host=True):
        if trace is not None:
            trace.append((name, np.array(ops.host(a) if host else a)))

    events = [None] * nc
    x0 = ops.downsample2(iq0); x1 = ops.downsample2(iq1)                       # TDownSample2: the even samples
    first = off // 2; nb = np.minimum(ns // 8, (int(x0.shape[0]) - off // 2) // 4)      # (sora_hip_ingest decimates whole groups of 8 raw samples of the BUFFER)
    note("x0", x0); note("x1", x1)
    # ---- TCCA11n behind RxSwitch
    st, used = ops.cca(x0, x1, u32(first), u32(nb), cca11n_states(nc), CCA11N_REARM)
    note("cca_state", st, False); note("cca_used", used, False)
    s0 = first + 4 * used.astype(np.int64); left = 4 * (nb - used.astype(np.int64))
    live = np.array([c for c in range(nc) if st[c, 0] == 1 and left[c] >= 368], np.int64)
    if len(live) == 0:
        return events
    s0 = s0[live]; left = left[live]; nl = len(live)
    # ---- L-LTF: TFreqEstimator_11n, TFreqComp_11n, 2 x 2 TFFT64, TSisoChannelEst
    vfo = ops.cfo_est(ops.take(x0, s0, 128), ops.take(x1, s0, 128))
    c0, c1 = ops.freq_comp(x0, x1, u32(s0), u32(np.full(nl, 16)), vfo)
    ch = ops.siso_est(ops.fft64(ops.take(c0, s0, 128)), ops.fft64(ops.take(c1, s0, 128)))
    note("vfo_lltf", vfo); note("ch", ch)
    # ---- L-SIG, HT-SIG 1 / 2: TFreqComp_11n, T11nDataSymbol, TFFT64, TSisoChannelComp + TMrcCombine, T11nSigDemap, the SIG decoder; the parser's gate
    c0, c1 = ops.freq_comp(x0, x1, u32(s0 + 128), u32(np.full(nl, 30)), vfo)
    y0, y1 = ops.data_symbol(c0, c1, u32(s0 + 128), u32(np.full(nl, 3)), u32(3 * np.arange(nl)), 3 * nl)
    note("sig_y0", y0); note("sig_y1", y1)
    mrc = ops.siso_comp_mrc(ch, ops.fft64(y0), ops.fft64(y1), u32(np.repeat(np.arange(nl), 3)))
    soft = ops.sig_demap(mrc)
    rec = ops.sig_decode(soft)
    note("sig_mrc", mrc); note("sig_soft", soft); note("sig_rec", rec, False)
    mcs = np.zeros(nl, np.int64); length = np.zeros(nl, np.int64); cr = np.zeros(nl, np.int64); nsym = np.zeros(nl, np.int64)
    go = []
    for j in range(nl):
        g = sig_gate11n(rec[j], mcs_max)
        if g is None:
            events[live[j]] = {"error_code": 0x80000005, "rate_kbps": 0, "length": 0, "crc32": 0, "mpdu": b""}
            continue
        mcs[j], length[j], cr[j], nsym[j] = g
        if left[j] >= 608 + 80 * nsym[j]:
            go.append(j)
    if not go:
        return events
    go = np.array(go, np.int64)
    # ---- HT-STF (dropped), HT-LTF 1 / 2: TMimoChannelEst
    nbur = np.zeros(nl, np.int64); nbur[go] = 30
    c0, c1 = ops.freq_comp(x0, x1, u32(s0 + 368), u32(nbur), vfo)
    y0, y1 = ops.data_symbol(c0, c1, u32(s0[go] + 448), u32(np.full(len(go), 2)), u32(2 * np.arange(len(go))), 2 * len(go))
    hinv = ops.mimo_est(ops.fft64(y0), ops.fft64(y1))
    note("hinv", hinv)
    # ---- the data field, symbol by symbol over the captures that still have one
    nbpsc = {8: 1, 9: 2, 10: 2, 11: 4, 12: 4, 13: 6, 14: 6}
    chunks = {int(j): [] for j in go}
    for k in range(int(nsym[go].max())):
        al = go[nsym[go] > k]                                                   # alive, as indices into the live captures; their rank in `go` finds their channel
        rank = np.searchsorted(go, al)
        nbur = np.zeros(nl, np.int64); nbur[al] = 10
        c0, c1 = ops.freq_comp(x0, x1, u32(s0 + 608 + 80 * k), u32(nbur), vfo)
        y0, y1 = ops.data_symbol(c0, c1, u32(s0[al] + 608 + 80 * k), u32(np.ones(len(al))), u32(np.arange(len(al))), len(al))
        e0, e1 = ops.mimo_comp(hinv, ops.fft64(y0), ops.fft64(y1), u32(rank))
        pf = np.zeros(nl, np.int64); pn = np.zeros(nl, np.int64); pf[al] = np.arange(len(al)); pn[al] = 1
        ops.pilot_track(e0, e1, u32(pf), u32(pn), vfo)
        for b in (1, 2, 4, 6):
            sel = np.array([i for i, j in enumerate(al) if nbpsc[int(mcs[j])] == b], np.int64)
            if len(sel) == 0:
                continue
            j0 = ops.demap_deint(ops.rows(e0, sel), b, 0); j1 = ops.demap_deint(ops.rows(e1, sel), b, 1)
            joined = ops.stream_join(j0, j1, b)
            if k == 0:
                note("joined0_nb%d" % b, joined)
            for i, r in enumerate(sel):
                chunks[int(al[r])].append(joined[i])
    note("vfo_end", vfo)
    # ---- T11aViterbi<5000 * 8, 312, 192, 36> per code rate, T11aDesc, TBB11aFrameSink
    for rate in (0, 1, 2):
        js = [int(j) for j in go if cr[j] == rate]
        if not js:
            continue
        nsoft = np.array([104 * nbpsc[int(mcs[j])] * nsym[j] for j in js], np.int64)
        soff = np.concatenate([[0], np.cumsum(nsoft)])[:-1]
        soft = ops.concat([p for j in js for p in chunks[j]])
        dec = ops.viterbi(soft, u32(soff), u32(nsoft), length[js], rate)
        boff = 1504 * np.arange(len(js))
        by = ops.desc(dec, u32(2560 * np.arange(len(js))), u32(length[js]), u32(boff), 1504 * len(js))
        srec = ops.frame_sink(by, u32(boff), u32(length[js]))
        hb = ops.host(by)
        note("mpdu_cr%d" % rate, by); note("sink_cr%d" % rate, srec, False)
        for i, j in enumerate(js):
            if srec[i, 0]:
                events[live[j]] = {"error_code": int(srec[i, 0]), "rate_kbps": int(mcs[j]), "length": int(length[j]), "crc32": int(srec[i, 1]),
                                   "mpdu": hb[boff[i]:boff[i] + length[j]].tobytes()}
    return events


def rx11n_by_stages(d_iq0, d_iq1, descs, mcs_max=10, trace=None):
    """The first event of every capture of a batch of two-chain 40 MHz captures, through the 802.11n stage entry points alone (rx11n_stages with the GPU's bricks):
    d_iq0 / d_iq1 int16 CUDA [samples, 2], descs [(first sample, samples)] -> per capture None or a dict error_code, rate_kbps (= MCS), length, crc32, mpdu.
    A DEMONSTRATION and a test vehicle, not a fast path: between stages it reads counts and records back to the host to build the next tables, and the data field costs
    some ten calls per OFDM symbol.  It does not reproduce the flush of zero-padded symbols at the end of a capture.  The fast path is Rx11n."""
    return rx11n_stages(_Gpu11nOps(d_iq0.device), d_iq0, d_iq1, descs, mcs_max, trace)


# ---- the front end of the 802.11a receive graph as stages (include/sora_hip.h, sora_hip_dc_remove11a .. sora_hip_plcp_parse11a)
# sora_cca11a_state as int32 words [n, 44]: 0 cca_state, 1 error_code, 2 cca_pwr_threshold, 3 cca_pwr_reading, 4 cca_peak_index, 5 sync_state, 6 auto_count, 7 sense_count,
# 8 high_count, 9 peak_corr, 10 peak_index, 12..27 sample_his (re | im << 16, oldest first, already >> 2), 28..31 / 32..35 / 36..39 the ac_re / ac_im / energy windows,
# oldest first, 40..42 their sums.  sora_dcest11a_state [n, 4]: 0 update_cnt, 1 sum_dc, 2 dc (packed).  sora_cs11a_state [n, 48]: the two, one behind the other.
CCA11A_WORDS, DCEST11A_WORDS, CS11A_WORDS = 44, 4, 48
CCA11A_STOP_ON_TIMEOUT = 1
E_CS_TIMEOUT = 0x80000007


def dcest11a_states(n):
    """-> int32 numpy [n, 4]: sora_dcest11a_state as constructed, in a fresh context: update_cnt 8, sum_dc 0, dc 0"""
    s = np.zeros((n, DCEST11A_WORDS), np.int32); s[:, 0] = 8
    return s


def cca11a_states(n, cca_pwr_threshold=1000 * 1000):
    """-> int32 numpy [n, 44]: sora_cca11a_state as a constructed TCCA11a holds it in a fresh context: all 0 but the threshold (the reference harness's by default)"""
    s = np.zeros((n, CCA11A_WORDS), np.int32); s[:, 2] = np.uint32(cca_pwr_threshold).astype(np.int32)
    return s


def cs11a_states(n, cca_pwr_threshold=1000 * 1000):
    """-> int32 numpy [n, 48]: sora_cs11a_state as constructed"""
    return np.concatenate([cca11a_states(n, cca_pwr_threshold), dcest11a_states(n)], axis=1)


def cca11a_reset(state, context=True):
    """Reset() on records (int32 numpy [n, 44] or [n, 48]), in place: TCCA11a::__init (and TDCEstimator::__init: update_cnt 8, sum_dc 0; dc stands); context: also
    what BB11aDemodContext::Reset / ResetCarrierSense clear, cca_state and error_code.  -> state"""
    state[:, 5:44] = 0
    if state.shape[1] == CS11A_WORDS:
        state[:, 44] = 8; state[:, 45] = 0
    if context:
        state[:, 0:2] = 0
    return state


def cs11a_record_words(state):
    """One sora_cs11a_state (48 words) -> words 0-39 of the receive handle's 64-word continuation record (Rx.stream_record_of; oracle.cs_trace) as uint32 [40].  Pure:
    a relabelling, with sum_dc and dc unpacked and sign-extended."""
    s = (np.asarray(state).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).reshape(CS11A_WORDS)
    w = np.zeros(40, np.uint32)
    w[0:16] = s[12:28]; w[16:28] = s[28:40]; w[28:31] = s[40:43]
    w[31] = s[7]; w[32] = s[8]; w[33] = s[9]; w[34] = s[10]; w[35] = s[44]
    for k, v in ((36, s[45]), (38, s[46])):
        h = np.array([v & 0xFFFF, v >> 16], np.uint16).view(np.int16).astype(np.int32).view(np.uint32)
        w[k] = h[0]; w[k + 1] = h[1]
    return w


def dc_remove11a(x, first, n, out_first, dc, out, max_n=None, stream=None):
    """TDCRemoveEx<4>: stream f = n[f] bursts of 4 from sample first[f] of x (int16 CUDA [samples, 2]) minus dc[f] (int16 CUDA [streams, 2]) -> out from sample out_first[f]"""
    _check(load().sora_hip_dc_remove11a(_dev_ptr(x), _dev_ptr(first), _dev_ptr(n), _dev_ptr(out_first), _dev_ptr(dc), _dev_ptr(out), first.shape[0], _max_n(n, max_n),
                                        _stream_ptr(stream)))
    return out


def dc_estimate11a(x, first, n, state, max_n=None, stream=None):
    """TDCEstimator: state int32 CUDA [streams, 4] (in / out) -> state"""
    _check(load().sora_hip_dc_estimate11a(_dev_ptr(x), _dev_ptr(first), _dev_ptr(n), _dev_ptr(state), first.shape[0], _max_n(n, max_n), _stream_ptr(stream)))
    return state


def cca11a(x, first, n, out_first, state, out, flags=0, max_n=None, stream=None):
    """TCCA11a over DC-removed bursts: x int16 CUDA [samples, 2] at 20 MHz; first (samples) / n (bursts) / out_first (BURSTS of out) int32 CUDA [streams]; state int32 CUDA
    [streams, 44] (in / out); out int16 CUDA [samples, 2] receives the gated bursts -> (used, npass) int32 CUDA [streams]"""
    import torch
    used = torch.zeros(first.shape[0], dtype=torch.int32, device=x.device); npass = torch.zeros_like(used)
    _check(load().sora_hip_cca11a(_dev_ptr(x), _dev_ptr(first), _dev_ptr(n), _dev_ptr(out_first), _dev_ptr(state), _dev_ptr(out), _dev_ptr(used), _dev_ptr(npass),
                                  first.shape[0], _max_n(n, max_n), int(flags), _stream_ptr(stream)))
    return used, npass


def carrier_sense11a(x, first, n, state, flags=0, max_n=None, stream=None):
    """TDCRemoveEx -> TCCA11a -> TDCEstimator over raw bursts: state int32 CUDA [streams, 48] (in / out) -> used int32 CUDA [streams]"""
    import torch
    used = torch.zeros(first.shape[0], dtype=torch.int32, device=x.device)
    _check(load().sora_hip_carrier_sense11a(_dev_ptr(x), _dev_ptr(first), _dev_ptr(n), _dev_ptr(state), _dev_ptr(used), first.shape[0], _max_n(n, max_n), int(flags),
                                            _stream_ptr(stream)))
    return used


def data_symbol11a(x, first, nsym, out_first, out, max_nsym=None, stream=None):
    """T11aDataSymbol: frame f's nsym[f] symbols of 80 samples from sample first[f] of x -> their samples 8..71 at symbol out_first[f] of out (int16 CUDA [symbols * 64, 2])"""
    _check(load().sora_hip_data_symbol11a(_dev_ptr(x), _dev_ptr(first), _dev_ptr(nsym), _dev_ptr(out_first), _dev_ptr(out), first.shape[0], _max_n(nsym, max_nsym),
                                          _stream_ptr(stream)))
    return out


def viterbi_sig11a(soft, stream=None):
    """T11aViterbiSig: soft uint8 CUDA [n, 48] -> int32 CUDA [n]: the decoded SIGNAL bits >> 6"""
    import torch
    sig = torch.zeros(soft.shape[0], dtype=torch.int32, device=soft.device)
    _check(load().sora_hip_viterbi_sig11a(_dev_ptr(soft), _dev_ptr(sig), soft.shape[0], _stream_ptr(stream)))
    return sig


def plcp_parse11a(sig, stream=None):
    """T11aPLCPParser: sig int32 CUDA [n] -> int32 CUDA [n, 5]: error_code, data_rate_kbps, frame_length, code_rate, total_symbols"""
    import torch
    rec = torch.zeros((sig.shape[0], 5), dtype=torch.int32, device=sig.device)
    _check(load().sora_hip_plcp_parse11a(_dev_ptr(sig), _dev_ptr(rec), sig.shape[0], _stream_ptr(stream)))
    return rec


class _Gpu11aOps:
    """rx11a_stages' bricks on the GPU: host tables and records (numpy) up, one stage call each, records back.  Buffers are torch CUDA tensors; a frame's context is
    [sora_lts11a_ctx row, sora_track11a_state row]."""

    def __init__(self, device):
        import torch
        self.torch = torch; self.dev = device

    def _up(self, a, dt=np.int32):
        return self.torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt, copy=False))).to(self.dev)

    def downsample2(self, iq):
        return ingest(iq, INGEST_DECIMATE2)

    def carrier_sense(self, x, first, n, state, flags):
        st = self._up(state)
        used = carrier_sense11a(x, self._up(first), self._up(n), st, flags, max_n=int(max(n)))
        return st.cpu().numpy(), used.cpu().numpy()

    def _take(self, x, starts, length):
        idx = (self._up(starts, np.int64)[:, None] + self.torch.arange(length, device=self.dev)[None, :]).reshape(-1)
        return x[idx].contiguous()

    def lts(self, x, starts):
        ctx = lts11a(self._take(x, starts, 144).reshape(-1, 144, 2))
        trk = np.zeros((len(starts), 134), np.int16); trk[:, 4] = 127; trk[:, 6::2] = 0x7FFF      # CF_PhaseCompensate / CF_PilotTrack after Reset (pilot.hpp:143-152)
        trk = self._up(trk, np.int16)
        return [[ctx[i:i + 1], trk[i:i + 1]] for i in range(len(starts))], ctx[:, 0].cpu().numpy()

    def symbols(self, x, starts, ctxs):
        n = len(starts)
        y = self.torch.zeros((n * 64, 2), dtype=self.torch.int16, device=self.dev)
        data_symbol11a(x, self._up(starts), self._up(np.ones(n)), self._up(np.arange(n)), y, max_nsym=1)
        ctx = self.torch.cat([c[0] for c in ctxs]).contiguous(); idx = self._up(np.arange(n))
        return equalize11a(fft64(freq_comp11a(y.reshape(n, 64, 2), ctx, idx)), ctx, idx)

    def track(self, eq, ctxs):
        n = len(ctxs)
        st = self.torch.cat([c[1] for c in ctxs]).contiguous(); idx = self._up(np.arange(n))
        out = pilot11a(phase_comp11a(eq, st, idx), idx, self._up(np.ones(n)), st)
        for i, c in enumerate(ctxs):
            c[1] = st[i:i + 1]
        return out

    def demap_deint(self, x, nb):
        return deinterleave11a(demap11a(x, nb), nb)

    def rows(self, a, idx):
        return a[self._up(idx, np.int64)].contiguous()

    def concat(self, parts):
        return self.torch.cat([p.reshape(-1) for p in parts]).contiguous()

    def viterbi_sig(self, soft):
        return viterbi_sig11a(soft)

    def plcp_parse(self, sig):
        return plcp_parse11a(sig).cpu().numpy().view(np.uint32)

    def viterbi(self, soft, soft_off, nsoft, lens, code_rate):
        return viterbi11a(soft, self._up(soft_off), self._up(nsoft), self._up(lens, np.int16), int(code_rate)).reshape(-1)

    def desc(self, dec, off, lens, out_off, total):
        out = self.torch.zeros(max(total, 1), dtype=self.torch.uint8, device=self.dev)
        return desc11a(dec, self._up(off), self._up(lens), out, self._up(out_off))

    def frame_sink(self, x, off, lens):
        return frame_sink11a(x, self._up(off), self._up(lens)).cpu().numpy().view(np.uint32)

    def host(self, a):
        return a.cpu().numpy()


def rx11a_stages(ops, iq, descs, sample_rate_mhz=40, cca_pwr_threshold=1000 * 1000):
    """The 802.11a receive graph (CreateDemodGraph11a_40M under RxThread, fb11a_demod.cpp:29-81) composed from the brick stages through `ops` (the GPU's:
    rx11a_by_stages; the model's: tests/rx11a_stage_model.ModelOps), along the walk of oracle/so_rx11a.c:691-768.  The host plays TMemSamples' source calls (14 samples at
    the 20 MHz rate, bursts of 4 as they fit), the routing bricks and RxThread: carrier sense runs with SORA_CCA11A_STOP_ON_TIMEOUT; the remaining bursts of the source call
    that raised the time-out run with it standing; then Reset.  After power_detected 144 samples go to lts11a, the SIGNAL symbol through the symbol stages, demap11a(1),
    deinterleave11a(1), viterbi_sig11a and plcp_parse11a, the data symbols by rate to viterbi11a, desc11a and frame_sink11a; then the frame reset, with the source's
    partial burst dropped (the next burst starts on the call grid).  Captures advance in rounds: each round is one call per stage over all captures in that phase.
    iq: the captures at 40 MHz (even offsets, whole 28-sample source calls) or at 20 MHz (whole 14-sample calls), descs [(first sample, samples)].
    -> per capture the list of EVERY event, dicts with the fields of the handle's rows: start_sample, end_sample, error_code, rate_kbps, length, nsym, crc32, cfo_est, mpdu.
    The 44 MHz graph's queue rule (TDownSample44_40 keeps its queue over a frame reset) is out of scope."""
    if sample_rate_mhz not in (40, 20):
        raise ValueError("rx11a_stages: 40 or 20 MHz (the 44 MHz graph's queue rule is not composed)")
    per = 2 if sample_rate_mhz == 40 else 1
    nc = len(descs)
    off = np.array([int(d[0]) for d in descs], np.int64); ns = np.array([int(d[1]) for d in descs], np.int64)
    if nc and ((ns % (14 * per)).any() or (off % per).any()):
        raise ValueError("rx11a_stages: a capture is whole source calls (28 samples at 40 MHz, 14 at 20) at an even offset")
    x = ops.downsample2(iq) if per == 2 else iq
    base = off // per; n20 = np.minimum(ns // per, int(x.shape[0]) - base)
    u32 = lambda a: np.asarray(a, np.int64).astype(np.uint32).view(np.int32)
    call_end = lambda p: (p + 13) // 14 * 14
    st = cs11a_states(nc, cca_pwr_threshold)
    p = np.zeros(nc, np.int64); phase = ["cs"] * nc; tail = np.zeros(nc, np.int64)
    events = [[] for _ in range(nc)]; fr = [dict() for _ in range(nc)]
    nbpsc = {6000: 1, 9000: 1, 12000: 2, 18000: 2, 24000: 4, 36000: 4, 48000: 6, 54000: 6}

    def frame_reset(c, at):
        p[c] = call_end(at); cca11a_reset(st[c:c + 1]); phase[c] = "cs" if p[c] + 4 <= n20[c] else "done"

    def fits(g, need):
        """the captures of g with `need(c)` more samples in them; the others end here without an event"""
        go = [c for c in g if p[c] + need(c) <= n20[c]]
        for c in g:
            if c not in go:
                phase[c] = "done"
        return go

    def sense(g):                                                                # ---- TDCRemoveEx -> TCCA11a -> TDCEstimator behind TBB11bRxSwitch
        s, used = ops.carrier_sense(x, u32(base[g] + p[g]), u32((n20[g] - p[g]) // 4), st[g], CCA11A_STOP_ON_TIMEOUT)
        for i, c in enumerate(g):
            st[c] = s[i]; p[c] += 4 * int(used[i])
            if st[c, 0] == 1:
                fr[c] = {"start": int(p[c])}; phase[c] = "lts"
            elif np.uint32(st[c, 1]) == E_CS_TIMEOUT:
                tail[c] = (min(call_end(p[c]), n20[c]) - p[c]) // 4; phase[c] = "tail"
            else:
                phase[c] = "done"

    def call_tail(g):                                                            # ---- the rest of the source call with the time-out standing, then ResetCarrierSense + Reset
        if tail[g].any():
            s, used = ops.carrier_sense(x, u32(base[g] + p[g]), u32(tail[g]), st[g], 0)
            for i, c in enumerate(g):
                st[c] = s[i]; p[c] += 4 * int(used[i])
        for c in g:
            cca11a_reset(st[c:c + 1]); phase[c] = "cs"

    def lts(g):                                                                  # ---- T11aSymSelEx -> T11aLTS
        go = fits(g, lambda c: 144)
        if go:
            ctxs, cfo = ops.lts(x, u32(base[go] + p[go]))
            for i, c in enumerate(go):
                fr[c]["ctx"] = ctxs[i]; fr[c]["cfo"] = int(cfo[i]); p[c] += 144; phase[c] = "sig"

    def signal(g):                                                               # ---- the SIGNAL symbol
        go = fits(g, lambda c: 80)
        if not go:
            return
        ctxs = [fr[c]["ctx"] for c in go]
        trk = ops.track(ops.symbols(x, u32(base[go] + p[go]), ctxs), ctxs)
        rec = ops.plcp_parse(ops.viterbi_sig(ops.demap_deint(trk, 1)))
        for i, c in enumerate(go):
            p[c] += 80
            if rec[i, 0]:                                                        # RxThread sees it at the end of the source call; the call's last bursts are consumed
                end = p[c] + (min(call_end(p[c]), n20[c]) - p[c]) // 4 * 4
                events[c].append({"start_sample": fr[c]["start"], "end_sample": int(end), "error_code": int(rec[i, 0]), "rate_kbps": 0, "length": 0, "nsym": 0,
                                  "crc32": 0, "cfo_est": fr[c]["cfo"], "mpdu": b""})
                frame_reset(c, p[c])
            else:
                fr[c].update(rate=int(rec[i, 1]), length=int(rec[i, 2]), cr=int(rec[i, 3]), nsym=int(rec[i, 4]) - 1); phase[c] = "data"

    def data(g):                                                                 # ---- the data symbols, by rate to the trellis, T11aDesc, TBB11aFrameSink
        go = fits(g, lambda c: 80 * fr[c]["nsym"])
        if not go:
            return
        chunks = {c: [] for c in go}
        for k in range(max(fr[c]["nsym"] for c in go)):
            al = [c for c in go if fr[c]["nsym"] > k]
            ctxs = [fr[c]["ctx"] for c in al]
            trk = ops.track(ops.symbols(x, u32(base[al] + p[al] + 80 * k), ctxs), ctxs)
            for b in (1, 2, 4, 6):
                sel = [i for i, c in enumerate(al) if nbpsc[fr[c]["rate"]] == b]
                if sel:
                    soft = ops.demap_deint(ops.rows(trk, sel), b)
                    for j, i in enumerate(sel):
                        chunks[al[i]].append(soft[j])
        for rate in (0, 1, 2):
            js = [c for c in go if fr[c]["cr"] == rate]
            if not js:
                continue
            nsoft = np.array([48 * nbpsc[fr[c]["rate"]] * fr[c]["nsym"] for c in js], np.int64)
            lens = np.array([fr[c]["length"] for c in js], np.int64)
            dec = ops.viterbi(ops.concat([q for c in js for q in chunks[c]]), u32(np.concatenate([[0], np.cumsum(nsoft)])[:-1]), u32(nsoft), lens, rate)
            boff = 2504 * np.arange(len(js))
            by = ops.desc(dec, u32(2560 * np.arange(len(js))), u32(lens), u32(boff), 2504 * len(js))
            srec = ops.frame_sink(by, u32(boff), u32(lens)); hb = ops.host(by)
            for i, c in enumerate(js):
                end = int(p[c] + 80 * fr[c]["nsym"])
                events[c].append({"start_sample": fr[c]["start"], "end_sample": end, "error_code": int(srec[i, 0]), "rate_kbps": fr[c]["rate"], "length": fr[c]["length"],
                                  "nsym": fr[c]["nsym"], "crc32": int(srec[i, 1]), "cfo_est": fr[c]["cfo"], "mpdu": hb[boff[i]:boff[i] + lens[i]].tobytes()})
                frame_reset(c, end)

    while True:                                                                  # a round: every capture takes the step of its phase, one call per stage over each group
        for c in range(nc):
            if phase[c] == "cs" and p[c] + 4 > n20[c]:
                phase[c] = "done"
        for name, step in (("cs", sense), ("tail", call_tail), ("lts", lts), ("sig", signal), ("data", data)):
            g = [c for c in range(nc) if phase[c] == name]
            if g:
                step(g)
        if all(ph == "done" for ph in phase):
            return events


def rx11a_by_stages(d_iq, descs, sample_rate_mhz=40, cca_pwr_threshold=1000 * 1000):
    """EVERY event of every capture of a batch, through the 802.11a stage entry points alone (rx11a_stages with the GPU's bricks): d_iq int16 CUDA [samples, 2] at 40 or
    20 MHz, descs [(first sample, samples)] -> per capture a list of dicts with the fields of the handle's rows.
    A DEMONSTRATION and a test vehicle, not a fast path: every round reads counts and records back to the host to build the next tables -- two carrier-sense calls and
    two round trips per time-out (every 21 bursts of silence), some eight calls per OFDM symbol.  Measured on 512 captures of one short frame each: 15 to 23 ms of host
    wall clock against 9 ms for Rx.process_dev + wait on the same batch; the rounds grow with the silence and the symbols of the longest capture.
    The 44 MHz graph's queue rule is out of scope.  The fast path is Rx."""
    return rx11a_stages(_Gpu11aOps(d_iq.device), d_iq, descs, sample_rate_mhz, cca_pwr_threshold)


def tx11n_samples(mpdu_len_nofcs, mcs):
    """Samples per TX chain of one 802.11n 2x2 frame (sora_hip_tx11n_samples); 0 for an unsupported MCS or length."""
    return int(load().sora_hip_tx11n_samples(int(mpdu_len_nofcs), int(mcs)))


def tx11n(mpdus, mcs, seeds=None, device=0, stream=None, sync=True, gaps=None):
    """Modulate a batch of MPDUs (bytes WITHOUT FCS) as 802.11n 2x2 frames on the GPU (MCS 8..14).
    -> (out0, out1, offsets): int16 CUDA tensors [total,2] COMPLEX16 @40 MHz for TX chains 0 and 1, and the offsets list.
    Frame f occupies samples offsets[f] .. offsets[f+1] of both (gaps[f] zero samples in front of frame f, if given, included at its start).
    seeds: scrambler seeds (None: 0xAB, the reference harness's).  A frame with an unsupported MCS or length is refused before any launch."""
    import torch
    n = len(mpdus)
    mcs = [int(m) for m in mcs] if np.ndim(mcs) else [int(mcs)] * n
    lens = [len(m) for m in mpdus]
    ns = [tx11n_samples(l, m) for l, m in zip(lens, mcs)]
    if len(mcs) != n or any(v == 0 for v in ns):
        raise SoraError(-1, "tx11n: unsupported MCS or length (MCS 8..14, 1..4092 bytes)")
    off = np.zeros(n + 1, np.int64); np.cumsum([(l + 3) // 4 * 4 for l in lens], out=off[1:])
    blob = np.zeros(max(int(off[-1]), 4), np.uint8)
    for f, m in enumerate(mpdus):
        blob[off[f]:off[f] + lens[f]] = np.frombuffer(bytes(m), np.uint8)
    gaps = [0] * n if gaps is None else [int(v) for v in gaps]
    ooff = np.zeros(n + 1, np.uint64); np.cumsum([a + b for a, b in zip(ns, gaps)], out=ooff[1:])
    first = ooff[:-1] + np.asarray(gaps, np.uint64)
    dev = torch.device("cuda", device)
    d_blob = torch.from_numpy(blob).to(dev); d_off = torch.from_numpy(off[:-1].astype(np.int32)).to(dev)
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).to(dev); d_mcs = torch.from_numpy(np.asarray(mcs, np.int32)).to(dev)
    d_seed = torch.from_numpy(np.asarray(seeds, np.uint8)).to(dev) if seeds is not None else None
    d_ooff = torch.from_numpy(first.astype(np.int64)).to(dev)
    out0 = torch.zeros((int(ooff[-1]), 2), dtype=torch.int16, device=dev)
    out1 = torch.zeros((int(ooff[-1]), 2), dtype=torch.int16, device=dev)
    _check(load().sora_hip_tx11n(_dev_ptr(d_blob), _dev_ptr(d_off), _dev_ptr(d_len), _dev_ptr(d_mcs), _dev_ptr(d_seed) if d_seed is not None else None, n,
                                 _dev_ptr(out0), _dev_ptr(out1), _dev_ptr(d_ooff), _stream_ptr(stream)))
    if sync:
        _check(load().sora_hip_stream_synchronize(_stream_ptr(stream)))
    return out0, out1, [int(v) for v in ooff]


# ---- the 802.11n modulation graphs' bricks as stages (include/sora_hip.h; bits packed in bytes, LSB first; N_b = ceil(52 n_bpsc / 8) bytes per stream and symbol)
def _row11n(n_bpsc):
    return (52 * int(n_bpsc) + 7) // 8


def stream_parse11n(s, n_bpsc, out=None, stream=None):
    """TStreamParser*_12: s uint8 CUDA [n, 13 n_bpsc] -> (uint8 CUDA [n, N_b], the same) for spatial streams 0 and 1; out: a pair of buffers to write into"""
    import torch
    n = s.shape[0]
    o0, o1 = out if out is not None else (torch.empty((n, _row11n(n_bpsc)), dtype=torch.uint8, device=s.device) for _ in range(2))
    _check(load().sora_hip_stream_parse11n(_dev_ptr(s), _dev_ptr(o0), _dev_ptr(o1), int(n_bpsc), n, _stream_ptr(stream)))
    return o0, o1


def interleave11n(s, n_bpsc, spatial_stream, out=None, stream=None):
    """T11nInterleave*_S1 / _S2 (spatial_stream 0 / 1): s uint8 CUDA [n, N_b] -> the same shape"""
    import torch
    out = torch.empty_like(s) if out is None else out
    _check(load().sora_hip_interleave11n(_dev_ptr(s), _dev_ptr(out), int(n_bpsc), int(spatial_stream), s.shape[0], _stream_ptr(stream)))
    return out


def map11n(s, n_bpsc, mod=0, out=None, stream=None):
    """TMap11a*<MOD> of the 802.11n graph: s uint8 CUDA [n, N_b] -> int16 CUDA [n, 52, 2]; mod = 0: 30339 / 21453 / 9594 / 4681"""
    import torch
    out = torch.empty((s.shape[0], 52, 2), dtype=torch.int16, device=s.device) if out is None else out
    _check(load().sora_hip_map11n(_dev_ptr(s), _dev_ptr(out), int(n_bpsc), int(mod), s.shape[0], _stream_ptr(stream)))
    return out


def sig_map11n(s, stream=None):
    """TSigMap11n: s uint8 CUDA [n, 18] -> int16 CUDA [n, 144, 2]"""
    import torch
    out = torch.empty((s.shape[0], 144, 2), dtype=torch.int16, device=s.device)
    _check(load().sora_hip_sig_map11n(_dev_ptr(s), _dev_ptr(out), s.shape[0], _stream_ptr(stream)))
    return out


def add_pilot11n(x, first, nsym, spatial_stream, pos0=None, out=None, stream=None):
    """T11nAddPilot<spatial_stream>: x int16 CUDA [n, 52, 2]; first / nsym (/ pos0) int32 CUDA [nframes] -> int16 CUDA [n, 64, 2]; symbols no frame owns stay
    as they were (0 in a buffer of the wrapper's)"""
    import torch
    out = torch.zeros((x.shape[0], 64, 2), dtype=torch.int16, device=x.device) if out is None else out
    _check(load().sora_hip_add_pilot11n(_dev_ptr(x), _dev_ptr(out), _dev_ptr(first), _dev_ptr(nsym), _opt_ptr(pos0), first.shape[0], int(spatial_stream),
                                        _stream_ptr(stream)))
    return out


def ifft_only11n(x, stream=None):
    """TIFFTxOnly: x int16 CUDA [n, 64, 2] -> int16 CUDA [n, 128, 2]"""
    import torch
    out = torch.empty((x.shape[0], 128, 2), dtype=torch.int16, device=x.device)
    _check(load().sora_hip_ifft_only11n(_dev_ptr(x), _dev_ptr(out), x.shape[0], _stream_ptr(stream)))
    return out


def csd11n(x, ncsd, stream=None):
    """TCSD<ncsd>: x int16 CUDA [n, 128, 2] -> the same shape, each symbol delayed circularly by 4 ncsd samples"""
    import torch
    out = torch.empty_like(x)
    _check(load().sora_hip_csd11n(_dev_ptr(x), _dev_ptr(out), int(ncsd), x.shape[0], _stream_ptr(stream)))
    return out


def add_gi11n(x, stream=None):
    """TAddGI: x int16 CUDA [n, 128, 2] -> int16 CUDA [n, 160, 2]"""
    import torch
    out = torch.empty((x.shape[0], 160, 2), dtype=torch.int16, device=x.device)
    _check(load().sora_hip_add_gi11n(_dev_ptr(x), _dev_ptr(out), x.shape[0], _stream_ptr(stream)))
    return out


def preamble11n(field, ncopies=1, device=0, stream=None):
    """LSrc (field 0) / HTSrc (field 1): -> (int16 CUDA [ncopies, 640 or 480, 2] for TX chain 0, the same for chain 1)"""
    import torch
    ns = {0: 640, 1: 480}.get(int(field), 640)
    o0, o1 = (torch.empty((int(ncopies), ns, 2), dtype=torch.int16, device=torch.device("cuda", device)) for _ in range(2))
    _check(load().sora_hip_preamble11n(_dev_ptr(o0), _dev_ptr(o1), int(field), int(ncopies), _stream_ptr(stream)))
    return o0, o1


_MCS_11N = {8: (1, CR_12, 52), 9: (2, CR_12, 104), 10: (2, CR_34, 156), 11: (4, CR_12, 208), 12: (4, CR_34, 312), 13: (6, CR_23, 416), 14: (6, CR_34, 468)}


def mod11n_fields(mpdu, mcs, seed=0xAB):
    """What TBB11nSigSrc and TBB11nSrc (PHY_11n.hpp:81-133, 251-278) send down the graphs for one MPDU without FCS: (the 9 SIG bytes: L-SIG at 6 Mbps with the LENGTH
    that spans the HT frame, then HT-SIG; SERVICE + MPDU + FCS + tail + pad -- ht_padding_bytes rounds N_SYM x N_DBPS bits up to whole bytes; the index of the tail
    byte; the symbols the graph emits once Flush has padded the encoder's last burst and the parser's last symbol with zeros; the scrambler register T11aSc starts from)"""
    import zlib
    nb, cr, nd = _MCS_11N[int(mcs)]
    mpdu = bytes(mpdu)
    ln = len(mpdu) + 4
    nstd = -(-(ln * 8 + 16 + 6) // nd)                                           # ht_symbol_count
    lsig = 0xB | ((((nstd + 5) * 24 - 16 - 6) // 8) << 5)
    lsig |= (bin(lsig).count("1") & 1) << 17
    ht = [int(mcs) & 0xFF, ln & 0xFF, (ln >> 8) & 0xFF, 3, 0, 0]
    crc = 0xFF                                                                   # CalcCRC8(cdata, 4, 2): reflected, poly 0xE0, over 34 bits, complemented
    for b in range(34):
        crc ^= (ht[b >> 3] >> (b & 7)) & 1
        crc = (crc >> 1) ^ 0xE0 if crc & 1 else crc >> 1
    crc = ~crc & 0xFF
    ht[4] |= (crc << 2) & 0xFF; ht[5] |= crc >> 6
    nbytes = (nstd * nd + 7) // 8
    data = np.zeros(nbytes, np.uint8)
    data[2:2 + len(mpdu)] = np.frombuffer(mpdu, np.uint8)
    data[2 + len(mpdu):2 + ln] = np.frombuffer(int(zlib.crc32(mpdu) & 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)
    ngroups = -(-nbytes // (cr + 1))
    nsym = -(-(cr + 2) * ngroups // (13 * nb))
    return np.array([lsig & 255, (lsig >> 8) & 255, (lsig >> 16) & 255] + ht, np.uint8), data, 2 + ln, nsym, int(seed) & 0xFF


class Mod11nStages:
    """sora_amd.tx11n's frames composed from stage entry points instead of the fused kernel: CreatePreambleGraph11n, CreateSigGraph11n and CreateModGraph11n
    (fb11nmod_config.hpp) brick by brick.  The constructor plays TBB11nSigSrc and TBB11nSrc on the host (mod11n_fields) and uploads the fields and the frame tables;
    run() is the stage chain, every intermediate through HBM.  The data symbols are laid out by modulation, so that each stage is one call per modulation, code rate
    or spatial stream whatever the batch; the three SIG symbols of every frame and both streams' data symbols share the IFFT and guard-interval calls; a last
    index_select puts the 160-sample blocks into frame order."""

    def __init__(self, mpdus, mcs, seeds=None, device=0):
        import torch
        n = self.n = len(mpdus)
        mcs = [int(m) for m in mcs] if np.ndim(mcs) else [int(mcs)] * n
        if len(mcs) != n or any(m not in _MCS_11N or not 1 <= len(p) <= 4092 for p, m in zip(mpdus, mcs)):
            raise SoraError(-1, "mod11n_by_stages: unsupported MCS or length (MCS 8..14, 1..4092 bytes)")
        seeds = [0xAB] * n if seeds is None else list(seeds)
        dev = self.dev = torch.device("cuda", device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        i32 = lambda a: up(np.asarray(a, np.int64).astype(np.int32), np.int32)
        fields = [mod11n_fields(p, m, s) for p, m, s in zip(mpdus, mcs, seeds)]
        par = [_MCS_11N[m] for m in mcs]
        nsym = [fl[3] for fl in fields]
        order = sorted(range(n), key=lambda f: (par[f][0], f))                   # data symbol slots, frames grouped by modulation
        slot0, at = [0] * n, 0
        for f in order:
            slot0[f] = at; at += nsym[f]
        self.nslots = at
        self.run_of, self.cbase, self.sbase, cat, sat = {}, {}, {}, 18 * n + (-18 * n) % 16, 0
        for nb in (1, 2, 4, 6):                                                  # n_bpsc -> (first slot, slots); the coded bytes (13 n_bpsc per slot) and the
            fs = [f for f in order if par[f][0] == nb]                           # stream bytes (N_b per slot) of a run lie together, from a 16-byte boundary
            cnt = sum(nsym[f] for f in fs)
            self.run_of[nb] = (slot0[fs[0]] if fs else at, cnt)
            self.cbase[nb] = cat; cat += (cnt * 13 * nb + 15) // 16 * 16
            self.sbase[nb] = sat; sat += (cnt * _row11n(nb) + 15) // 16 * 16
        self.coded_bytes, self.stream_bytes = cat, max(sat, 16)
        # the uncoded bytes: the SIG fields (9 bytes each), then the data fields, each with room for the zeros Flush pads the encoder's last burst with
        glen = [-(-len(fl[1]) // (p[1] + 1)) * (p[1] + 1) for fl, p in zip(fields, par)]
        doff = np.zeros(n + 1, np.int64); np.cumsum(glen, out=doff[1:]); doff += 9 * n
        raw = np.zeros(int(doff[-1]), np.uint8)
        for f, fl in enumerate(fields):
            raw[9 * f:9 * f + 9] = fl[0]; raw[doff[f]:doff[f] + len(fl[1])] = fl[1]
        self.d_raw = up(raw, np.uint8)
        dlen = [len(fl[1]) for fl in fields]
        self.scr = (i32(doff[:-1]), i32(dlen), i32([fl[2] for fl in fields]), up(np.asarray([fl[4] for fl in fields], np.uint8), np.uint8), max(dlen))
        # TConvEncode_*: the SIG fields at rate 1/2 (18 bytes each from byte 0 of the coded buffer), the data fields by code rate; a fresh register per field
        self.enc = [(CR_12, i32([9 * f for f in range(n)]), i32([9] * n), i32([18 * f for f in range(n)]), n, 9)]
        for cr in (CR_12, CR_23, CR_34):
            fs = [f for f in range(n) if par[f][1] == cr]
            if fs:
                self.enc.append((cr, i32([doff[f] for f in fs]), i32([glen[f] for f in fs]),
                                 i32([self.cbase[par[f][0]] + (slot0[f] - self.run_of[par[f][0]][0]) * 13 * par[f][0] for f in fs]), len(fs), max(glen[f] for f in fs)))
        self.sig_pil = (i32([3 * f for f in range(n)]), i32([3] * n))           # T11aAddPilot<30339>: L-SIG is position 0 of its three symbols
        self.pil = (i32(slot0), i32(nsym))                                       # T11nAddPilot: the first data symbol is position 0
        # 160-sample blocks of a chain's buffer: n x 4 of LSrc, 3 n SIG symbols, the data slots, n x 3 of HTSrc; frame order: L, SIG, HT, data
        ht0 = 7 * n + self.nslots
        blocks = []
        for f in range(n):
            blocks += list(range(4 * f, 4 * f + 4)) + list(range(4 * n + 3 * f, 4 * n + 3 * f + 3)) + list(range(ht0 + 3 * f, ht0 + 3 * f + 3))
            blocks += list(range(7 * n + slot0[f], 7 * n + slot0[f] + nsym[f]))
        self.d_blocks = up(np.asarray(blocks, np.int64), np.int64)
        offs = np.zeros(n + 1, np.int64); np.cumsum([1600 + 160 * k for k in nsym], out=offs[1:])
        self.offsets = [int(v) for v in offs]

    def run(self):
        """-> (out0, out1): int16 CUDA [total, 2] per TX chain; everything in order on torch's current stream (the gather at the end is torch's), nothing waited for"""
        import torch
        L = load()
        st = _stream_ptr(None)
        n, dev, ns = self.n, self.dev, self.nslots
        u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)
        i16 = lambda *shape: torch.empty(shape + (2,), dtype=torch.int16, device=dev)
        off, ln, tail, seed, mx = self.scr
        d_scr = scramble11a(self.d_raw, off, ln, seed, tail=tail, max_len=mx)    # (the SIG bytes and the encoder's pad bytes are in no frame of the call)
        d_coded = u8(self.coded_bytes)                                           # zeros: what Flush pads the parser's last symbol with
        for cr, in_off, ilen, out_off, cnt, mxl in self.enc:
            _check(L.sora_hip_conv_encode11a(_dev_ptr(d_scr), _dev_ptr(in_off), _dev_ptr(ilen), cr, _dev_ptr(d_coded), _dev_ptr(out_off), cnt, mxl, st))
        # bins of every symbol that goes through TIFFTxOnly: 3 n SIG symbols, the data slots of stream 0, those of stream 1
        d_bins = i16(3 * n + 2 * ns, 64)
        d_sig = interleave11a(d_coded[:18 * n].view(3 * n, 6), 1)
        d_sigcar = sig_map11n(d_sig.view(n, 18))
        _check(L.sora_hip_add_pilot11a_from(_dev_ptr(d_sigcar), _dev_ptr(d_bins), _dev_ptr(self.sig_pil[0]), _dev_ptr(self.sig_pil[1]), None, n, 30339, st))
        d_par = [u8(self.stream_bytes), u8(self.stream_bytes)]
        d_int = [u8(self.stream_bytes), u8(self.stream_bytes)]
        d_car = i16(2 * ns, 52)
        for nb in (1, 2, 4, 6):                                                  # TStreamParser* -> T11nInterleave*_S1 / _S2 -> TMap11a*, per modulation
            s0, cnt = self.run_of[nb]
            if cnt:
                sb = self.sbase[nb]
                _check(L.sora_hip_stream_parse11n(d_coded.data_ptr() + self.cbase[nb], d_par[0].data_ptr() + sb, d_par[1].data_ptr() + sb, nb, cnt, st))
                for iss in (0, 1):
                    _check(L.sora_hip_interleave11n(d_par[iss].data_ptr() + sb, d_int[iss].data_ptr() + sb, nb, iss, cnt, st))
                    _check(L.sora_hip_map11n(d_int[iss].data_ptr() + sb, d_car.data_ptr() + (iss * ns + s0) * 208, nb, 0, cnt, st))
        for iss in (0, 1):                                                       # (every slot belongs to a frame)
            _check(L.sora_hip_add_pilot11n(d_car.data_ptr() + iss * ns * 208, d_bins.data_ptr() + (3 * n + iss * ns) * 256, _dev_ptr(self.pil[0]),
                                           _dev_ptr(self.pil[1]), None, n, iss, st))
        d_t = ifft_only11n(d_bins)
        d_c = i16(3 * n + ns, 128)                                               # chain 1 before its guard interval: TCSD<2> of the SIG symbols, TCSD<4> of stream 1
        _check(L.sora_hip_csd11n(d_t.data_ptr(), d_c.data_ptr(), 2, 3 * n, st))
        if ns:
            _check(L.sora_hip_csd11n(d_t.data_ptr() + (3 * n + ns) * 512, d_c.data_ptr() + 3 * n * 512, 4, ns, st))
        outs = []
        for ch, src in enumerate((d_t, d_c)):                                    # a chain's blocks: LSrc, SIG + data behind TAddGI, HTSrc
            outs.append(i16(10 * n + ns, 160))
            _check(L.sora_hip_add_gi11n(src.data_ptr(), outs[ch].data_ptr() + 4 * n * 640, 3 * n + ns, st))
        _check(L.sora_hip_preamble11n(outs[0].data_ptr(), outs[1].data_ptr(), 0, n, st))
        _check(L.sora_hip_preamble11n(outs[0].data_ptr() + (7 * n + ns) * 640, outs[1].data_ptr() + (7 * n + ns) * 640, 1, n, st))
        return tuple(o.index_select(0, self.d_blocks).reshape(-1, 2) for o in outs)


def mod11n_by_stages(mpdus, mcs, seeds=None, device=0, sync=True):
    """Modulate a batch of MPDUs (bytes WITHOUT FCS) through the stage chain (Mod11nStages) -> (out0, out1, offsets): the same as sora_amd.tx11n returns."""
    plan = Mod11nStages(mpdus, mcs, seeds, device)
    out0, out1 = plan.run()
    if sync:
        _check(load().sora_hip_stream_synchronize(_stream_ptr(None)))
    return out0, out1, plan.offsets


def tx_ht40_samples(mpdu_len_nofcs, mcs, mcs_max=14, gi=0, joint=False):
    """Samples per TX chain of one 40 MHz HT 2x2 frame (sora_hip_tx_ht40_samples): 1280 + 160 (2 + N_SYM); 0 for an MCS or length that is not accepted.
    mcs_max other than 14, a kind gi or joint=True: sora_hip_tx_ht40_mcs_samples / _joint_mcs_samples (mcs_max=15 accepts MCS 15; gi 1: 1600 + 144 N_SYM)."""
    if mcs_max == 14 and not gi and not joint:
        return int(load().sora_hip_tx_ht40_samples(int(mpdu_len_nofcs), int(mcs)))
    fn = load().sora_hip_tx_ht40_joint_mcs_samples if joint else load().sora_hip_tx_ht40_mcs_samples
    return int(fn(int(mpdu_len_nofcs), int(mcs), int(gi) & 0xFFFFFFFF, int(mcs_max)))


def tx_ht40_gi_samples(mpdu_len_nofcs, mcs, gi):
    """Samples per TX chain of one 40 MHz HT 2x2 frame of guard-interval kind gi (sora_hip_tx_ht40_gi_samples): 0 = long, 1600 + 160 N_SYM; 1 = short, 1600 + 144 N_SYM;
    0 for a kind, MCS or length that is not accepted."""
    return int(load().sora_hip_tx_ht40_gi_samples(int(mpdu_len_nofcs), int(mcs), int(gi) & 0xFFFFFFFF))


def _tx_gi(gi, n, who):
    """gi=None -> None (the entry point without a kind); else one kind (0 long / 1 short) per frame as a list"""
    if gi is None:
        return None
    g = [int(v) for v in gi] if np.ndim(gi) else [int(gi)] * n
    if len(g) != n or any(v not in (0, 1) for v in g):
        raise SoraError(-1, who + ": gi must hold one guard-interval kind per frame, 0 (long) or 1 (short)")
    return g


def tx_ht40(mpdus0, mpdus1, mcs, seeds=None, device=0, stream=None, sync=True, gaps=None, gi=None, mcs_max=14):
    """Modulate a batch of MPDU pairs (bytes WITHOUT FCS; mpdus0[f] on spatial stream 0, mpdus1[f] on stream 1, of equal length) as HT-mixed
    40 MHz two-stream frames on the GPU (MCS 8..14): what RxHt40 receives.
    -> (out0, out1, offsets): int16 CUDA tensors [total,2] COMPLEX16 @40 MHz for TX chains 0 and 1, and the offsets list.
    Frame f occupies samples offsets[f] .. offsets[f+1] of both (gaps[f] zero samples in front of frame f, if given, included at its start);
    its HT-LTF 1 starts 1280 samples after its first sample.
    seeds: one (seed0, seed1) pair of scrambler seeds per frame (None: 0x5D, 0x2B).  A frame that is not accepted is refused before any launch.
    gi: None -> sora_hip_tx_ht40; else one guard-interval kind per frame (or one for all), 0 = long, 1 = short (data symbols of 144 samples, HT-SIG bit 31) ->
    sora_hip_tx_ht40_gi.  mcs_max: 14, or 15 -> sora_hip_tx_ht40_mcs with that gate (gi None: all long): MCS 15 (64-QAM, rate 5/6) is accepted as well; any other value
    is refused."""
    import torch
    n = len(mpdus0)
    mcs = [int(m) for m in mcs] if np.ndim(mcs) else [int(mcs)] * n
    lens = [len(m) for m in mpdus0]
    if len(mpdus1) != n or len(mcs) != n or any(len(b) != l for b, l in zip(mpdus1, lens)):
        raise SoraError(-1, "tx_ht40: one MPDU per stream and frame, both of a frame of the same length")
    gi = _tx_gi(gi, n, "tx_ht40")
    gated = mcs_max != 14
    if gated:
        if mcs_max != 15:
            raise SoraError(-1, "tx_ht40: mcs_max is 14 or 15")
        gi = [0] * n if gi is None else gi
        ns = [tx_ht40_samples(l, m, mcs_max, g) for l, m, g in zip(lens, mcs, gi)]
    else:
        ns = [tx_ht40_samples(l, m) for l, m in zip(lens, mcs)] if gi is None else [tx_ht40_gi_samples(l, m, g) for l, m, g in zip(lens, mcs, gi)]
    if any(v == 0 for v in ns):
        raise SoraError(-1, "tx_ht40: unsupported MCS or length (MCS 8..14, or ..15 with mcs_max=15; 1..3996 bytes)")
    if seeds is not None and (len(seeds) != n or any(len(p) != 2 for p in seeds)):
        raise SoraError(-1, "tx_ht40: seeds must hold one pair per frame")
    off = np.zeros(2 * n + 1, np.int64); np.cumsum([(l + 3) // 4 * 4 for l in lens for _ in range(2)], out=off[1:])
    blob = np.zeros(max(int(off[-1]), 4), np.uint8)
    for f in range(n):
        blob[off[2 * f]:off[2 * f] + lens[f]] = np.frombuffer(bytes(mpdus0[f]), np.uint8)
        blob[off[2 * f + 1]:off[2 * f + 1] + lens[f]] = np.frombuffer(bytes(mpdus1[f]), np.uint8)
    gaps = [0] * n if gaps is None else [int(v) for v in gaps]
    ooff = np.zeros(n + 1, np.uint64); np.cumsum([a + b for a, b in zip(ns, gaps)], out=ooff[1:])
    first = ooff[:-1] + np.asarray(gaps, np.uint64)
    dev = torch.device("cuda", device)
    d_blob = torch.from_numpy(blob).to(dev); d_off = torch.from_numpy(off[:-1].astype(np.int32)).to(dev)
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).to(dev); d_mcs = torch.from_numpy(np.asarray(mcs, np.int32)).to(dev)
    d_seed = torch.from_numpy(np.asarray(seeds, np.int64).astype(np.uint8).reshape(-1)).to(dev) if seeds is not None else None
    d_ooff = torch.from_numpy(first.astype(np.int64)).to(dev)
    out0 = torch.zeros((int(ooff[-1]), 2), dtype=torch.int16, device=dev)
    out1 = torch.zeros((int(ooff[-1]), 2), dtype=torch.int16, device=dev)
    if gated:
        d_gi = torch.from_numpy(np.asarray(gi, np.uint8)).to(dev)
        _check(load().sora_hip_tx_ht40_mcs(_dev_ptr(d_blob), _dev_ptr(d_off), _dev_ptr(d_len), _dev_ptr(d_mcs), _dev_ptr(d_seed) if d_seed is not None else None,
                                           _dev_ptr(d_gi), n, _dev_ptr(out0), _dev_ptr(out1), _dev_ptr(d_ooff), int(mcs_max), _stream_ptr(stream)))
    elif gi is None:
        _check(load().sora_hip_tx_ht40(_dev_ptr(d_blob), _dev_ptr(d_off), _dev_ptr(d_len), _dev_ptr(d_mcs), _dev_ptr(d_seed) if d_seed is not None else None, n,
                                       _dev_ptr(out0), _dev_ptr(out1), _dev_ptr(d_ooff), _stream_ptr(stream)))
    else:
        d_gi = torch.from_numpy(np.asarray(gi, np.uint8)).to(dev)
        _check(load().sora_hip_tx_ht40_gi(_dev_ptr(d_blob), _dev_ptr(d_off), _dev_ptr(d_len), _dev_ptr(d_mcs), _dev_ptr(d_seed) if d_seed is not None else None,
                                          _dev_ptr(d_gi), n, _dev_ptr(out0), _dev_ptr(out1), _dev_ptr(d_ooff), _stream_ptr(stream)))
    if sync:
        _check(load().sora_hip_stream_synchronize(_stream_ptr(stream)))
    return out0, out1, [int(v) for v in ooff]


def tx_ht40_joint_samples(mpdu_len_nofcs, mcs):
    """Samples per TX chain of one joint-coded 40 MHz HT 2x2 frame (sora_hip_tx_ht40_joint_samples): 1280 + 160 (2 + N_SYM); 0 for an MCS or length that is not accepted."""
    return int(load().sora_hip_tx_ht40_joint_samples(int(mpdu_len_nofcs), int(mcs)))


def tx_ht40_joint_gi_samples(mpdu_len_nofcs, mcs, gi):
    """as tx_ht40_gi_samples, for one joint-coded frame (sora_hip_tx_ht40_joint_gi_samples)"""
    return int(load().sora_hip_tx_ht40_joint_gi_samples(int(mpdu_len_nofcs), int(mcs), int(gi) & 0xFFFFFFFF))


def tx_ht40_joint(mpdus, mcs, seeds=None, device=0, stream=None, sync=True, gaps=None, gi=None, mcs_max=14):
    """Modulate a batch of MPDUs (bytes WITHOUT FCS), ONE per frame, as joint-coded HT-mixed 40 MHz two-stream frames on the GPU (MCS 8..14): what an RxHt40 in
    CODING_JOINT receives.  -> (out0, out1, offsets) as tx_ht40.  seeds: one scrambler seed per frame (None: 0x5D).  A frame that is not accepted is refused before
    any launch.  gi: as tx_ht40's (None -> sora_hip_tx_ht40_joint; else sora_hip_tx_ht40_joint_gi).  mcs_max: as tx_ht40's (15 -> sora_hip_tx_ht40_joint_mcs)."""
    import torch
    n = len(mpdus)
    mcs = [int(m) for m in mcs] if np.ndim(mcs) else [int(mcs)] * n
    lens = [len(m) for m in mpdus]
    if len(mcs) != n:
        raise SoraError(-1, "tx_ht40_joint: one MCS per frame")
    gi = _tx_gi(gi, n, "tx_ht40_joint")
    gated = mcs_max != 14
    if gated:
        if mcs_max != 15:
            raise SoraError(-1, "tx_ht40_joint: mcs_max is 14 or 15")
        gi = [0] * n if gi is None else gi
        ns = [tx_ht40_samples(l, m, mcs_max, g, joint=True) for l, m, g in zip(lens, mcs, gi)]
    else:
        ns = [tx_ht40_joint_samples(l, m) for l, m in zip(lens, mcs)] if gi is None else [tx_ht40_joint_gi_samples(l, m, g) for l, m, g in zip(lens, mcs, gi)]
    if any(v == 0 for v in ns):
        raise SoraError(-1, "tx_ht40_joint: unsupported MCS or length (MCS 8..14, or ..15 with mcs_max=15; 1..3996 bytes)")
    if seeds is not None and (len(seeds) != n or any(np.ndim(p) != 0 for p in seeds)):
        raise SoraError(-1, "tx_ht40_joint: seeds must hold one seed per frame")
    off = np.zeros(n + 1, np.int64); np.cumsum([(l + 3) // 4 * 4 for l in lens], out=off[1:])
    blob = np.zeros(max(int(off[-1]), 4), np.uint8)
    for f in range(n):
        blob[off[f]:off[f] + lens[f]] = np.frombuffer(bytes(mpdus[f]), np.uint8)
    gaps = [0] * n if gaps is None else [int(v) for v in gaps]
    ooff = np.zeros(n + 1, np.uint64); np.cumsum([a + b for a, b in zip(ns, gaps)], out=ooff[1:])
    first = ooff[:-1] + np.asarray(gaps, np.uint64)
    dev = torch.device("cuda", device)
    d_blob = torch.from_numpy(blob).to(dev); d_off = torch.from_numpy(off[:-1].astype(np.int32)).to(dev)
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).to(dev); d_mcs = torch.from_numpy(np.asarray(mcs, np.int32)).to(dev)
    d_seed = torch.from_numpy(np.asarray(seeds, np.int64).astype(np.uint8).reshape(-1)).to(dev) if seeds is not None else None
    d_ooff = torch.from_numpy(first.astype(np.int64)).to(dev)
    out0 = torch.zeros((int(ooff[-1]), 2), dtype=torch.int16, device=dev)
    out1 = torch.zeros((int(ooff[-1]), 2), dtype=torch.int16, device=dev)
    if gated:
        d_gi = torch.from_numpy(np.asarray(gi, np.uint8)).to(dev)
        _check(load().sora_hip_tx_ht40_joint_mcs(_dev_ptr(d_blob), _dev_ptr(d_off), _dev_ptr(d_len), _dev_ptr(d_mcs), _dev_ptr(d_seed) if d_seed is not None else None,
                                                 _dev_ptr(d_gi), n, _dev_ptr(out0), _dev_ptr(out1), _dev_ptr(d_ooff), int(mcs_max), _stream_ptr(stream)))
    elif gi is None:
        _check(load().sora_hip_tx_ht40_joint(_dev_ptr(d_blob), _dev_ptr(d_off), _dev_ptr(d_len), _dev_ptr(d_mcs), _dev_ptr(d_seed) if d_seed is not None else None, n,
                                             _dev_ptr(out0), _dev_ptr(out1), _dev_ptr(d_ooff), _stream_ptr(stream)))
    else:
        d_gi = torch.from_numpy(np.asarray(gi, np.uint8)).to(dev)
        _check(load().sora_hip_tx_ht40_joint_gi(_dev_ptr(d_blob), _dev_ptr(d_off), _dev_ptr(d_len), _dev_ptr(d_mcs), _dev_ptr(d_seed) if d_seed is not None else None,
                                                _dev_ptr(d_gi), n, _dev_ptr(out0), _dev_ptr(out1), _dev_ptr(d_ooff), _stream_ptr(stream)))
    if sync:
        _check(load().sora_hip_stream_synchronize(_stream_ptr(stream)))
    return out0, out1, [int(v) for v in ooff]


# ---- the 40 MHz HT modulation graph's bricks as stages (include/sora_hip.h; bits packed in bytes, LSB first; N_b40 = ceil(108 n_bpsc / 8) bytes per stream and symbol)
def _row_ht40(n_bpsc):
    return (108 * int(n_bpsc) + 7) // 8


def stream_parse_ht40(s, n_bpsc, out=None, stream=None):
    """the stream parser: s uint8 CUDA [n, 27 n_bpsc] -> (uint8 CUDA [n, N_b40], the same) for spatial streams 0 and 1; out: a pair of buffers to write into"""
    import torch
    n = s.shape[0]
    o0, o1 = out if out is not None else (torch.empty((n, _row_ht40(n_bpsc)), dtype=torch.uint8, device=s.device) for _ in range(2))
    _check(load().sora_hip_stream_parse_ht40(_dev_ptr(s), _dev_ptr(o0), _dev_ptr(o1), int(n_bpsc), n, _stream_ptr(stream)))
    return o0, o1


def interleave_ht40(s, n_bpsc, spatial_stream, out=None, stream=None):
    """the HT interleaver for 40 MHz: s uint8 CUDA [n, N_b40] -> the same shape"""
    import torch
    out = torch.empty_like(s) if out is None else out
    _check(load().sora_hip_interleave_ht40(_dev_ptr(s), _dev_ptr(out), int(n_bpsc), int(spatial_stream), s.shape[0], _stream_ptr(stream)))
    return out


def interleave_ht40_stream(s, in_off, first, nsym, n_bpsc, spatial_stream, out, stream=None):
    """the same map reading by bit address: s uint8 CUDA [nbytes]; in_off / first / nsym int32 CUDA [nframes]; symbol j of frame f reads bits 108 n_bpsc j onward of
    s[in_off[f]:] and writes row first[f] + j of out (uint8 CUDA [rows, N_b40], written in place and returned); no other row is touched"""
    _check(load().sora_hip_interleave_ht40_stream(_dev_ptr(s), _dev_ptr(in_off), _dev_ptr(first), _dev_ptr(nsym), _dev_ptr(out), int(n_bpsc), int(spatial_stream),
                                                  in_off.shape[0], _stream_ptr(stream)))
    return out


def map_ht40(s, n_bpsc, out=None, stream=None):
    """the mapper: s uint8 CUDA [n, N_b40] -> int16 CUDA [n, 108, 2]: odd integers times 6144 / 6144 / 4000 / 2214"""
    import torch
    out = torch.empty((s.shape[0], 108, 2), dtype=torch.int16, device=s.device) if out is None else out
    _check(load().sora_hip_map_ht40(_dev_ptr(s), _dev_ptr(out), int(n_bpsc), s.shape[0], _stream_ptr(stream)))
    return out


def sig_map_ht40(s, out=None, stream=None):
    """L-SIG + HT-SIG: s uint8 CUDA [n, 18] -> int16 CUDA [n, 3, 128, 2]: three complete symbols of bins per frame"""
    import torch
    out = torch.empty((s.shape[0], 3, 128, 2), dtype=torch.int16, device=s.device) if out is None else out
    _check(load().sora_hip_sig_map_ht40(_dev_ptr(s), _dev_ptr(out), s.shape[0], _stream_ptr(stream)))
    return out


def add_pilot_ht40(x, first, nsym, out=None, stream=None):
    """x int16 CUDA [n, 108, 2]; first / nsym int32 CUDA [nframes] -> int16 CUDA [n, 128, 2]; symbols no frame owns stay as they were (0 in a buffer of the wrapper's)"""
    import torch
    out = torch.zeros((x.shape[0], 128, 2), dtype=torch.int16, device=x.device) if out is None else out
    _check(load().sora_hip_add_pilot_ht40(_dev_ptr(x), _dev_ptr(out), _dev_ptr(first), _dev_ptr(nsym), first.shape[0], _stream_ptr(stream)))
    return out


def ifft_ht40(x, out=None, stream=None):
    """the fixed-point IFFT<128>, natural order: x int16 CUDA [n, 128, 2] -> the same shape"""
    import torch
    out = torch.empty_like(x) if out is None else out
    _check(load().sora_hip_ifft_ht40(_dev_ptr(x), _dev_ptr(out), x.shape[0], _stream_ptr(stream)))
    return out


def add_gi_ht40(x, gi=0, out=None, stream=None):
    """the guard interval: x int16 CUDA [n, 128, 2] -> int16 CUDA [n, 160, 2] (gi 0) or [n, 144, 2] (gi 1)"""
    import torch
    out = torch.empty((x.shape[0], 144 if int(gi) == 1 else 160, 2), dtype=torch.int16, device=x.device) if out is None else out
    _check(load().sora_hip_add_gi_ht40(_dev_ptr(x), _dev_ptr(out), int(gi), x.shape[0], _stream_ptr(stream)))
    return out


def preamble_ht40(field, ncopies=1, device=0, stream=None):
    """field 0: L-STF, L-LTF; field 1: HT-STF, HT-LTF1, HT-LTF2 -> (int16 CUDA [ncopies, 640 or 480, 2] for TX chain 0, the same for chain 1)"""
    import torch
    ns = {0: 640, 1: 480}.get(int(field), 640)
    o0, o1 = (torch.empty((int(ncopies), ns, 2), dtype=torch.int16, device=torch.device("cuda", device)) for _ in range(2))
    _check(load().sora_hip_preamble_ht40(_dev_ptr(o0), _dev_ptr(o1), int(field), int(ncopies), _stream_ptr(stream)))
    return o0, o1


_MCS_HT40 = {8: (1, CR_12, 54), 9: (2, CR_12, 108), 10: (2, CR_34, 162), 11: (4, CR_12, 216), 12: (4, CR_34, 324), 13: (6, CR_23, 432), 14: (6, CR_34, 486)}


def mod_ht40_fields(mpdus, mcs, coding=HT40_CODING_PER_STREAM, gi=0, seeds=None):
    """The host's share of one frame of the 40 MHz HT modulation chains.  mpdus: (mpdu0, mpdu1) WITHOUT FCS (per-stream coding) or one MPDU (joint).
    -> (the 9 SIG bytes: L-SIG at 6 Mbps with the LENGTH that spans the HT frame, HT-SIG with the short-GI bit and its CRC-8; a list of one field per encoder: SERVICE +
    PSDU + FCS + tail + pad up to N_SYM x N_DBPS bits, then zeros up to the encoder stage's whole bursts; the bytes of a field that are scrambled; the index of the tail
    byte; per field the register sora_hip_scramble11a starts from -- the seed's seven bits reversed, << 1: seed bit i is x[-1 - i]; N_SYM).
    seeds: (s0, s1) / one seed; None: 0x5D, 0x2B / 0x5D."""
    import zlib
    nb, cr, nd = _MCS_HT40[int(mcs)]
    joint = int(coding) == HT40_CODING_JOINT
    ms = [bytes(mpdus)] if joint else [bytes(mpdus[0]), bytes(mpdus[1])]
    if joint:
        nd *= 2
    gi = int(gi)
    ln = len(ms[0]) + 4
    nsym = -(-(16 + 8 * ln + 6) // nd)
    lsig = 0xB | ((12 + 3 * ((9 * nsym + 9) // 10 if gi else nsym)) << 5)
    lsig |= (bin(lsig).count("1") & 1) << 17
    h4 = (int(mcs) & 0x7F) | (1 << 7) | ((ln & 0xFFFF) << 8) | (7 << 24) | (gi << 31)
    crc = 0xFF                                                                   # CRC-8 over HT-SIG bits 0..33: reflected, poly 0xE0, complemented
    for b in range(34):
        crc ^= (h4 >> b) & 1
        crc = (crc >> 1) ^ 0xE0 if crc & 1 else crc >> 1
    sig = lsig | ((h4 | ((~crc & 0xFF) << 34)) << 24)
    nbytes = (nsym * nd + 7) // 8
    data = []
    for mp in ms:
        d = np.zeros(-(-nbytes // (cr + 1)) * (cr + 1), np.uint8)
        d[2:2 + len(mp)] = np.frombuffer(mp, np.uint8)
        d[2 + len(mp):2 + ln] = np.frombuffer(int(zlib.crc32(mp) & 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)
        data.append(d)
    if seeds is None:
        seeds = (0x5D,) if joint else (0x5D, 0x2B)
    seeds = [seeds] if np.ndim(seeds) == 0 else list(seeds)
    regs = [int("{:07b}".format(int(s) & 0x7F)[::-1], 2) << 1 for s in seeds]
    return np.frombuffer(sig.to_bytes(9, "little"), np.uint8).copy(), data, nbytes, 2 + ln, regs, nsym


class ModHt40Stages:
    """sora_amd.tx_ht40's / tx_ht40_joint's frames composed from stage entry points instead of the fused kernels (include/sora_hip.h: the chains of the 40 MHz HT
    modulation graph).  The constructor plays the source on the host (mod_ht40_fields) and uploads the fields and the frame tables; run() is the stage chain, every
    intermediate through HBM.  The data symbols are laid out by guard-interval kind, then modulation, so that each stage is one call per kind, modulation, code rate or
    spatial stream whatever the batch; the SIG symbols and both streams' data symbols share one IFFT call; a last index_select over blocks of 160 samples (of 16 where a batch holds short symbols) puts
    the fields into frame order.  Joint coding: the encoder stage emits whole bursts, so at MCS 8, 10 and 14 a frame of an odd number of symbols ends one or two coded bytes behind
    its last symbol's row; such a frame gets one more row, a symbol that no frame owns and nothing reads."""

    def __init__(self, mpdus0, mpdus1, mcs, seeds=None, gi=None, device=0):
        import torch
        n = self.n = len(mpdus0)
        joint = self.joint = mpdus1 is None
        who = "mod_ht40_by_stages"
        mcs = [int(m) for m in mcs] if np.ndim(mcs) else [int(mcs)] * n
        lens = [len(p) for p in mpdus0]
        if len(mcs) != n or (not joint and (len(mpdus1) != n or any(len(b) != l for b, l in zip(mpdus1, lens)))):
            raise SoraError(-1, who + ": one MCS per frame; one MPDU per stream and frame, both of a frame of the same length")
        if any(m not in _MCS_HT40 or not 1 <= l <= 3996 for l, m in zip(lens, mcs)):
            raise SoraError(-1, who + ": unsupported MCS or length (MCS 8..14, 1..3996 bytes)")
        if seeds is not None and (len(seeds) != n or any((np.ndim(p) != 0) if joint else (np.ndim(p) != 1 or len(p) != 2) for p in seeds)):
            raise SoraError(-1, who + ": seeds must hold one seed (joint coding) or one pair (per-stream coding) per frame")
        g = _tx_gi(gi, n, who) or [0] * n
        dev = self.dev = torch.device("cuda", device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        i32 = lambda a: up(np.asarray(a, np.int64).astype(np.int32), np.int32)
        coding = HT40_CODING_JOINT if joint else HT40_CODING_PER_STREAM
        fields = [mod_ht40_fields(mpdus0[f] if joint else (mpdus0[f], mpdus1[f]), mcs[f], coding, g[f], None if seeds is None else seeds[f]) for f in range(n)]
        par = [_MCS_HT40[m] for m in mcs]
        nsym = [fl[5] for fl in fields]
        nfld = 1 if joint else 2
        out_len = [len(fl[1][0]) // (p[1] + 1) * (p[1] + 2) for fl, p in zip(fields, par)]      # coded bytes the encoder stage writes per field
        rows = [-(-o // (27 * p[0])) if joint else k for o, p, k in zip(out_len, par, nsym)]    # data symbol slots a frame takes
        order = sorted(range(n), key=lambda f: (g[f], par[f][0], f))             # slots: long frames then short ones, each grouped by modulation
        slot0, at = [0] * n, 0
        for f in order:
            slot0[f] = at; at += rows[f]
        ns = self.nslots = at
        self.nlong = sum(rows[f] for f in range(n) if g[f] == 0)
        self.runs, cat, sat = [], 18 * n + (-18 * n) % 16, 0                     # (n_bpsc, first slot, slots, coded base, stream base): bases on 16-byte boundaries
        for kind in (0, 1):
            for nb in (1, 2, 4, 6):
                fs = [f for f in order if g[f] == kind and par[f][0] == nb]
                cnt = sum(rows[f] for f in fs)
                if cnt:
                    self.runs.append((nb, slot0[fs[0]], cnt, cat, sat, fs))
                    if joint:
                        cat += (cnt * 27 * nb + 15) // 16 * 16
                    sat += (cnt * _row_ht40(nb) + 15) // 16 * 16
        self.stream_bytes = max(sat, 16)
        coded_off = [[0] * nfld for _ in range(n)]
        for nb, s0, cnt, cb, sb, fs in self.runs:
            for f in fs:
                if joint:
                    coded_off[f][0] = cb + (slot0[f] - s0) * 27 * nb
                else:                                                            # per-stream coding: the coded streams lie one behind the other, read by bit address
                    for s in (0, 1):
                        coded_off[f][s] = cat; cat += out_len[f]
        self.coded_bytes = cat + 16
        # the uncoded bytes: the SIG fields (9 bytes each), then the data fields, each with its zeros up to the encoder's whole bursts
        flds = [(f, s) for f in range(n) for s in range(nfld)]
        glen = [len(fields[f][1][s]) for f, s in flds]
        doff = np.zeros(len(flds) + 1, np.int64); np.cumsum(glen, out=doff[1:]); doff += 9 * n
        raw = np.zeros(int(doff[-1]), np.uint8)
        for f, fl in enumerate(fields):
            raw[9 * f:9 * f + 9] = fl[0]
        for k, (f, s) in enumerate(flds):
            raw[doff[k]:doff[k] + glen[k]] = fields[f][1][s]
        self.d_raw = up(raw, np.uint8)
        self.scr = (i32(doff[:-1]), i32([fields[f][2] for f, s in flds]), i32([fields[f][3] for f, s in flds]),
                    up(np.asarray([fields[f][4][s] for f, s in flds], np.uint8), np.uint8), max(fields[f][2] for f in range(n)))
        # the encoder: the SIG fields at rate 1/2 (18 bytes each from byte 0 of the coded buffer), the data fields by code rate; a fresh register per field
        self.enc = [(CR_12, i32([9 * f for f in range(n)]), i32([9] * n), i32([18 * f for f in range(n)]), n, 9)]
        for cr in (CR_12, CR_23, CR_34):
            ks = [k for k, (f, s) in enumerate(flds) if par[f][1] == cr]
            if ks:
                self.enc.append((cr, i32([doff[k] for k in ks]), i32([glen[k] for k in ks]), i32([coded_off[flds[k][0]][flds[k][1]] for k in ks]), len(ks),
                                 max(glen[k] for k in ks)))
        if not joint:                                                            # interleave_ht40_stream's tables per run and stream: (byte offsets, first rows, symbols)
            self.ist = [[(i32([coded_off[f][s] for f in fs]), i32([slot0[f] - s0 for f in fs]), i32([nsym[f] for f in fs])) for s in (0, 1)]
                        for nb, s0, cnt, cb, sb, fs in self.runs]
        self.pil = (i32(slot0), i32(nsym))
        # blocks of a chain's buffer, of 160 samples, or of 16 where a short symbol (144) is among them: n x 640 samples of L-STF + L-LTF, 3 n x 160 of SIG, n x 480 of
        # HT-STF + HT-LTFs, the long slots x 160, the short slots x 144
        u = self.block = 16 if any(g) else 160
        pl, ps, sl, ss = 640 // u, 480 // u, 160 // u, 144 // u
        blocks, offs = [], [0]
        for f in range(n):
            blocks += list(range(pl * f, pl * f + pl)) + list(range(pl * n + ps * f, pl * n + ps * f + ps)) + list(range((pl + ps) * n + ps * f, (pl + ps) * n + ps * f + ps))
            b0 = (pl + 2 * ps) * n + (sl * slot0[f] if g[f] == 0 else sl * self.nlong + ss * (slot0[f] - self.nlong))
            blocks += list(range(b0, b0 + (ss if g[f] else sl) * nsym[f]))
            offs.append(offs[-1] + 1600 + (144 if g[f] else 160) * nsym[f])
        self.d_blocks = up(np.asarray(blocks, np.int64), np.int64)
        self.offsets = offs

    def run(self):
        """-> (out0, out1): int16 CUDA [total, 2] per TX chain; everything in order on torch's current stream (the gather at the end is torch's), nothing waited for"""
        import torch
        L = load()
        st = _stream_ptr(None)
        n, dev, ns, nl = self.n, self.dev, self.nslots, self.nlong
        u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)
        i16 = lambda *shape: torch.empty(shape + (2,), dtype=torch.int16, device=dev)
        off, ln, tail, seed, mx = self.scr
        d_scr = scramble11a(self.d_raw, off, ln, seed, tail=tail, max_len=mx)    # (the SIG bytes and the encoder's pad bytes are in no frame of the call)
        d_coded = u8(self.coded_bytes)
        for cr, in_off, ilen, out_off, cnt, mxl in self.enc:
            _check(L.sora_hip_conv_encode11a(_dev_ptr(d_scr), _dev_ptr(in_off), _dev_ptr(ilen), cr, _dev_ptr(d_coded), _dev_ptr(out_off), cnt, mxl, st))
        # bins of every symbol that goes through the IFFT: 3 n SIG symbols, the data slots of stream 0, those of stream 1
        d_bins = i16(3 * n + 2 * ns, 128)
        d_sig = interleave11a(d_coded[:18 * n].view(3 * n, 6), 1)
        _check(L.sora_hip_sig_map_ht40(_dev_ptr(d_sig), d_bins.data_ptr(), n, st))
        d_int = [u8(self.stream_bytes), u8(self.stream_bytes)]
        d_par = [u8(self.stream_bytes), u8(self.stream_bytes)] if self.joint else None
        d_car = i16(2 * ns, 108)
        for r, (nb, s0, cnt, cb, sb, fs) in enumerate(self.runs):
            if self.joint:
                _check(L.sora_hip_stream_parse_ht40(d_coded.data_ptr() + cb, d_par[0].data_ptr() + sb, d_par[1].data_ptr() + sb, nb, cnt, st))
            for iss in (0, 1):
                if self.joint:
                    _check(L.sora_hip_interleave_ht40(d_par[iss].data_ptr() + sb, d_int[iss].data_ptr() + sb, nb, iss, cnt, st))
                else:
                    io, fi, nsy = self.ist[r][iss]
                    _check(L.sora_hip_interleave_ht40_stream(d_coded.data_ptr(), _dev_ptr(io), _dev_ptr(fi), _dev_ptr(nsy), d_int[iss].data_ptr() + sb, nb, iss, len(fs), st))
                _check(L.sora_hip_map_ht40(d_int[iss].data_ptr() + sb, d_car.data_ptr() + (iss * ns + s0) * 432, nb, cnt, st))
        for iss in (0, 1):
            _check(L.sora_hip_add_pilot_ht40(d_car.data_ptr() + iss * ns * 432, d_bins.data_ptr() + (3 * n + iss * ns) * 512, _dev_ptr(self.pil[0]), _dev_ptr(self.pil[1]),
                                             n, st))
        d_t = ifft_ht40(d_bins)
        total = 1600 * n + 160 * nl + 144 * (ns - nl)                            # samples of a chain's buffer: L, SIG, HT, long slots, short slots
        outs = [i16(total), i16(total)]
        for ch in (0, 1):                                                        # one add_gi call per chain and kind; the SIG symbols are the same on both chains
            src = d_t.data_ptr() + (3 * n + ch * ns) * 512
            _check(L.sora_hip_add_gi_ht40(d_t.data_ptr(), outs[ch].data_ptr() + 640 * n * 4, 0, 3 * n, st))
            _check(L.sora_hip_add_gi_ht40(src, outs[ch].data_ptr() + 1600 * n * 4, 0, nl, st))
            _check(L.sora_hip_add_gi_ht40(src + nl * 512, outs[ch].data_ptr() + (1600 * n + 160 * nl) * 4, 1, ns - nl, st))
        _check(L.sora_hip_preamble_ht40(outs[0].data_ptr(), outs[1].data_ptr(), 0, n, st))
        _check(L.sora_hip_preamble_ht40(outs[0].data_ptr() + 1120 * n * 4, outs[1].data_ptr() + 1120 * n * 4, 1, n, st))
        return tuple(o.view(-1, self.block, 2).index_select(0, self.d_blocks).reshape(-1, 2) for o in outs)


def mod_ht40_by_stages(mpdus0, mpdus1, mcs, seeds=None, gi=None, device=0, sync=True):
    """Modulate a batch through the stage chain (ModHt40Stages).  mpdus1 a list: per-stream coding, what sora_amd.tx_ht40(mpdus0, mpdus1, mcs, seeds, gi=gi) returns;
    mpdus1 None: joint coding, what sora_amd.tx_ht40_joint(mpdus0, mcs, seeds, gi=gi) returns.  -> (out0, out1, offsets)"""
    plan = ModHt40Stages(mpdus0, mpdus1, mcs, seeds, gi, device)
    out0, out1 = plan.run()
    if sync:
        _check(load().sora_hip_stream_synchronize(_stream_ptr(None)))
    return out0, out1, plan.offsets


TX11B_RATES = (1000, 2000, 5500, 11000)


def tx11b_samples(mpdu_len_nofcs, rate_kbps, preamble=0):
    """Samples of one 802.11b frame (sora_hip_tx11b_pre_samples; preamble 0 = long, 1 = short); 0 for an unsupported rate, length or kind
    (1000 kbps behind the short preamble is one)."""
    return int(load().sora_hip_tx11b_pre_samples(int(mpdu_len_nofcs), int(rate_kbps), int(preamble) & 0xFFFFFFFF))


def _tx11b_frames(mpdus, rates_kbps, phase_in, preamble):
    """what tx11b and mod11b_by_stages accept -> (n, rates, lengths, kinds or None, samples per frame, phase_in as a list or None); the rest is refused"""
    n = len(mpdus)
    rates = [int(r) for r in rates_kbps] if np.ndim(rates_kbps) else [int(rates_kbps)] * n
    lens = [len(m) for m in mpdus]
    kinds = None
    if preamble is not None:
        kinds = [int(k) for k in preamble] if np.ndim(preamble) else [int(preamble)] * n
        if len(kinds) != n or any(k not in (0, 1) for k in kinds):
            raise SoraError(-1, "tx11b: preamble must hold one kind, 0 (long) or 1 (short), per frame")
    ns = [tx11b_samples(l, r, k) for l, r, k in zip(lens, rates, kinds or [0] * n)]
    if len(rates) != n or any(v == 0 for v in ns):
        raise SoraError(-1, "tx11b: unsupported rate, length or preamble (1000/2000/5500/11000 kbps, 1..4092 bytes; no 1000 kbps behind the short preamble)")
    if phase_in is not None:
        phase_in = [int(p) for p in phase_in] if np.ndim(phase_in) else [int(phase_in)] * n
        if len(phase_in) != n or any(not 0 <= p <= 3 for p in phase_in):
            raise SoraError(-1, "tx11b: phase_in must hold one value 0..3 per frame")
    return n, rates, lens, kinds, ns, phase_in


def tx11b(mpdus, rates_kbps, phase_in=None, device=0, stream=None, sync=True, gaps=None, return_phase=False, preamble=None):
    """Modulate a batch of MPDUs (bytes WITHOUT FCS) as 802.11b frames on the GPU (1000, 2000, 5500, 11000 kbps).  preamble: None = every frame behind the
    long preamble (sora_hip_tx11b); else 0 (long) or 1 (short: 2000, 5500, 11000 kbps only), one value or one per frame (sora_hip_tx11b_pre).
    -> (out, offsets): an int8 CUDA tensor [total,2] COMPLEX8 @44 MHz and the offsets list; frame f occupies samples offsets[f] ..
    offsets[f+1] (gaps[f] zero samples in front of frame f, if given, included at its start).
    phase_in: the reference's last_phase (0..3) at the start of each frame, one value or one per frame (None: 0, a fresh reference
    process).  return_phase: also return last_phase after each frame, a list -- pass it back as phase_in to continue one reference
    process's sequence.  A frame with an unsupported rate or length is refused before any launch."""
    import torch
    n, rates, lens, kinds, ns, phase_in = _tx11b_frames(mpdus, rates_kbps, phase_in, preamble)
    off = np.zeros(n + 1, np.int64); np.cumsum([(l + 3) // 4 * 4 for l in lens], out=off[1:])
    blob = np.zeros(max(int(off[-1]), 4), np.uint8)
    for f, m in enumerate(mpdus):
        blob[off[f]:off[f] + lens[f]] = np.frombuffer(bytes(m), np.uint8)
    gaps = [0] * n if gaps is None else [int(v) for v in gaps]
    ooff = np.zeros(n + 1, np.uint64); np.cumsum([a + b for a, b in zip(ns, gaps)], out=ooff[1:])
    first = ooff[:-1] + np.asarray(gaps, np.uint64)
    dev = torch.device("cuda", device)
    d_blob = torch.from_numpy(blob).to(dev); d_off = torch.from_numpy(off[:-1].astype(np.int32)).to(dev)
    d_len = torch.from_numpy(np.asarray(lens, np.int32)).to(dev); d_rate = torch.from_numpy(np.asarray(rates, np.int32)).to(dev)
    d_pin = torch.from_numpy(np.asarray(phase_in, np.uint8)).to(dev) if phase_in is not None else None
    d_pout = torch.zeros(n, dtype=torch.uint8, device=dev) if return_phase else None
    d_ooff = torch.from_numpy(first.astype(np.int64)).to(dev)
    out = torch.zeros((int(ooff[-1]), 2), dtype=torch.int8, device=dev)
    tail = (_dev_ptr(d_pin) if d_pin is not None else None, _dev_ptr(d_pout) if d_pout is not None else None, n, _dev_ptr(out), _dev_ptr(d_ooff), _stream_ptr(stream))
    if kinds is None:
        _check(load().sora_hip_tx11b(_dev_ptr(d_blob), _dev_ptr(d_off), _dev_ptr(d_len), _dev_ptr(d_rate), *tail))
    else:
        d_kind = torch.from_numpy(np.asarray(kinds, np.uint8)).to(dev)
        _check(load().sora_hip_tx11b_pre(_dev_ptr(d_blob), _dev_ptr(d_off), _dev_ptr(d_len), _dev_ptr(d_rate), _dev_ptr(d_kind), *tail))
    if sync:
        _check(load().sora_hip_stream_synchronize(_stream_ptr(stream)))
    if return_phase:
        return out, [int(v) for v in ooff], [int(v) for v in d_pout.cpu().numpy()]
    return out, [int(v) for v in ooff]


# ---- the 802.11b modulation graph's bricks as stages (include/sora_hip.h: sora_hip_ppdu11b .. sora_hip_pulse_shape11b) -----------------------------
# Records, as int32 words per stream: the spreaders' [n, 4] last_phase, is_even, reserved x 2 (sora_mod11b_state); the scrambler's [n] register; the shaper's
# [n, 16] m_temps[0..3] as packed COMPLEX16 (sora_shaper11b_state).  Offsets and counts are int32 CUDA [streams].
MOD11B_CHIPS_PER_BYTE = {1000: 88, 2000: 44, 5500: 16, 11000: 8}


def ppdu11b(mpdu, off, length, rate_kbps, preamble, out, out_first, stream=None):
    """TBB11bSrc: mpdu uint8 CUDA; off / length / rate_kbps / out_first int32 CUDA [frames]; preamble uint8 CUDA [frames] (0 long, 1 short) -> out uint8 CUDA, frame f's
    PPDU bytes (24 or 15 + length + 4) from byte out_first[f] written in place; a frame that is not accepted gets nothing written"""
    _check(load().sora_hip_ppdu11b(_dev_ptr(mpdu), _dev_ptr(off), _dev_ptr(length), _dev_ptr(rate_kbps), _dev_ptr(preamble), _dev_ptr(out), _dev_ptr(out_first), off.shape[0],
                                   _stream_ptr(stream)))
    return out


def _mod11b(fn, x, first, n, out_first, state, out, max_n, stream):
    _check(getattr(load(), fn)(_dev_ptr(x), _dev_ptr(first), _dev_ptr(n), _dev_ptr(out_first), _dev_ptr(state), _dev_ptr(out), first.shape[0], _max_n(n, max_n),
                               _stream_ptr(stream)))
    return out


def sc741_11b(x, first, n, out_first, reg, out, max_n=None, stream=None):
    """TSc741: n[f] bytes from byte first[f] of x (uint8 CUDA) -> out (from byte out_first[f]); reg int32 CUDA [streams] (the 7-bit register, in / out)"""
    return _mod11b("sora_hip_sc741_11b", x, first, n, out_first, reg, out, max_n, stream)


def dbpsk_spread11b(x, first, n, out_first, state, out, max_n=None, stream=None):
    """TBB11bDBPSKSpread: n[f] bytes -> 88 n[f] chips, out int8 CUDA [chips, 2] from chip out_first[f]; state int32 CUDA [streams, 4] (last_phase in / out)"""
    return _mod11b("sora_hip_dbpsk_spread11b", x, first, n, out_first, state, out, max_n, stream)


def dqpsk_spread11b(x, first, n, out_first, state, out, max_n=None, stream=None):
    """TBB11bDQPSKSpread: n[f] bytes -> 44 n[f] chips (as dbpsk_spread11b)"""
    return _mod11b("sora_hip_dqpsk_spread11b", x, first, n, out_first, state, out, max_n, stream)


def cck5_encode11b(x, first, n, out_first, state, out, max_n=None, stream=None):
    """TCCK5Encode: n[f] bytes -> 16 n[f] chips; state: last_phase"""
    return _mod11b("sora_hip_cck5_encode11b", x, first, n, out_first, state, out, max_n, stream)


def cck11_encode11b(x, first, n, out_first, state, out, max_n=None, stream=None):
    """TCCK11Encode: n[f] bytes -> 8 n[f] chips; state: last_phase and is_even"""
    return _mod11b("sora_hip_cck11_encode11b", x, first, n, out_first, state, out, max_n, stream)


def pulse_shape11b(x, first, n, out_first, state, out, flush=None, max_n=None, stream=None):
    """TQuickPulseShaper: x int8 CUDA [chips, 2]; n[f] chips from chip first[f] -> out int16 CUDA [samples, 2], 4 n[f] samples from sample out_first[f] (4 (n[f] + 5) where
    flush[f], uint8 CUDA [streams], is not 0: the brick's Flush); state int32 CUDA [streams, 16] (m_temps[0..3], in / out)"""
    _check(load().sora_hip_pulse_shape11b(_dev_ptr(x), _dev_ptr(first), _dev_ptr(n), _dev_ptr(out_first), _opt_ptr(flush), _dev_ptr(state), _dev_ptr(out), first.shape[0],
                                          _max_n(n, max_n), _stream_ptr(stream)))
    return out


class Mod11bStages:
    """The 802.11b modulation graph composed from its stage entry points, for a batch of MPDUs (bytes WITHOUT FCS): ppdu11b -> sc741_11b -> the host's TBB11bMRSelect
    (the header's bytes to the DBPSK stage -- behind the short preamble its six PLCP bytes to the DQPSK stage --, MPDU + FCS to the stage of the frame's rate, all on one
    last_phase record per frame) -> pulse_shape11b with Flush -> the last burst of eight padded with zeros -> pack16to8.  The constructor refuses what tx11b refuses,
    lays the batch out and uploads it; run() is the launches alone (up to ten) and may be repeated.  offsets: as tx11b's; state[:, 0]: last_phase after each frame."""

    def __init__(self, mpdus, rates_kbps, phase_in=None, preamble=None, device=0):
        import torch
        n, rates, lens, kinds, ns, phase_in = _tx11b_frames(mpdus, rates_kbps, phase_in, preamble)
        kinds = kinds or [0] * n
        dev = torch.device("cuda", device)

        def i32(v):                                                               # (offsets are unsigned 32-bit words on the device)
            return torch.from_numpy(np.asarray(v, np.int64).astype(np.uint32).view(np.int32)).to(dev)

        hb1 = np.asarray([24 if k == 0 else 9 for k in kinds], np.int64)          # header bytes through the DBPSK spreader, then through the DQPSK one
        hb2 = np.asarray([0 if k == 0 else 6 for k in kinds], np.int64)
        pay = np.asarray(lens, np.int64) + 4
        cpb = np.asarray([MOD11B_CHIPS_PER_BYTE[r] for r in rates], np.int64)
        moff = np.zeros(n + 1, np.int64); np.cumsum([(l + 3) // 4 * 4 for l in lens], out=moff[1:])
        blob = np.zeros(max(int(moff[-1]), 4), np.uint8)
        for f, m in enumerate(mpdus):
            blob[moff[f]:moff[f] + lens[f]] = np.frombuffer(bytes(m), np.uint8)
        poff = np.zeros(n + 1, np.int64); np.cumsum(hb1 + hb2 + pay, out=poff[1:])   # PPDU bytes
        nchips = 88 * hb1 + 44 * hb2 + pay * cpb
        coff = np.zeros(n + 1, np.int64); np.cumsum(nchips, out=coff[1:])
        soff = np.zeros(n + 1, np.int64); np.cumsum(ns, out=soff[1:])               # samples: 4 (chips + 5) and four of padding
        assert all(int(a) == 4 * int(b) + 24 for a, b in zip(ns, nchips))
        if int(soff[-1]) >= 1 << 32:
            raise SoraError(-6, "Mod11bStages: the batch's samples must stay below 2^32 (the stages' offsets are 32-bit)")
        self.n, self.offsets = n, [int(v) for v in soff]
        self._blob, self._moff, self._lens, self._rates = torch.from_numpy(blob).to(dev), i32(moff[:-1]), i32(lens), i32(rates)
        self._kinds = torch.from_numpy(np.asarray(kinds, np.uint8)).to(dev)
        self._poff, self._nppdu = i32(poff[:-1]), i32(hb1 + hb2 + pay)
        self._reg0 = i32([0x6C if k == 0 else 0x1B for k in kinds])               # DOT11B_PLCP_{LONG,SHORT}_TX_SCRAMBLER_REGISTER
        self._state0 = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        if phase_in is not None:
            self._state0[:, 0] = i32(phase_in)
        # TBB11bMRSelect: a stream of 0 bytes leaves the record alone, so every call takes all frames and the frame's own segments carry its last_phase on
        self._calls = [(dbpsk_spread11b, i32(poff[:-1]), i32(hb1), i32(coff[:-1]), int(hb1.max()))]
        if hb2.any():
            self._calls.append((dqpsk_spread11b, i32(poff[:-1] + hb1), i32(hb2), i32(coff[:-1] + 88 * hb1), 6))
        for rate, fn in ((1000, dbpsk_spread11b), (2000, dqpsk_spread11b), (5500, cck5_encode11b), (11000, cck11_encode11b)):
            sel = np.asarray([r == rate for r in rates])
            if sel.any():
                self._calls.append((fn, i32(poff[:-1] + hb1 + hb2), i32(np.where(sel, pay, 0)), i32(coff[:-1] + 88 * hb1 + 44 * hb2), int(pay[sel].max())))
        self._coff, self._nchips, self._soff = i32(coff[:-1]), i32(nchips), i32(soff[:-1])
        self._max_ppdu, self._max_chips = int((hb1 + hb2 + pay).max()), int(nchips.max())
        self._flush = torch.ones(n, dtype=torch.uint8, device=dev)
        self.ppdu = torch.zeros(int(poff[-1]), dtype=torch.uint8, device=dev)
        self.scrambled = torch.zeros_like(self.ppdu)
        self.reg = self._reg0.clone(); self.state = self._state0.clone()
        self.shaper = torch.zeros((n, 16), dtype=torch.int32, device=dev)
        self.chips = torch.zeros((int(coff[-1]), 2), dtype=torch.int8, device=dev)
        self.wide = torch.zeros((int(soff[-1]), 2), dtype=torch.int16, device=dev)    # (the padding behind each frame's flush stays 0)
        self.out = torch.empty((int(soff[-1]), 2), dtype=torch.int8, device=dev)

    def run(self, stream=None):
        """-> int8 CUDA [total, 2], the same as sora_amd.tx11b returns; the records start afresh with every run"""
        self.reg.copy_(self._reg0); self.state.copy_(self._state0); self.shaper.zero_()
        ppdu11b(self._blob, self._moff, self._lens, self._rates, self._kinds, self.ppdu, self._poff, stream)
        sc741_11b(self.ppdu, self._poff, self._nppdu, self._poff, self.reg, self.scrambled, self._max_ppdu, stream)
        for fn, first, cnt, out_first, max_n in self._calls:
            fn(self.scrambled, first, cnt, out_first, self.state, self.chips, max_n, stream)
        pulse_shape11b(self.chips, self._coff, self._nchips, self._soff, self.shaper, self.wide, self._flush, self._max_chips, stream)
        _check(load().sora_hip_pack16to8(_dev_ptr(self.wide), _dev_ptr(self.out), self.wide.shape[0], _stream_ptr(stream)))
        return self.out


def mod11b_by_stages(mpdus, rates_kbps, phase_in=None, preamble=None, device=0, sync=True):
    """The 802.11b modulation graph composed from its stage entry points (Mod11bStages) for a batch of MPDUs (bytes WITHOUT FCS): the host does TBB11bMRSelect's
    routing for both preamble kinds and pads the last burst of TPackSample16to8.
    -> (out, offsets, phase_out): what sora_amd.tx11b(mpdus, rates_kbps, phase_in, return_phase=True, preamble=preamble) returns, and it refuses what tx11b refuses,
    before any launch.  A demonstration of the stages, up to ten launches and every intermediate through HBM: not a fast path (that is tx11b)."""
    plan = Mod11bStages(mpdus, rates_kbps, phase_in, preamble, device)
    out = plan.run()
    if sync:
        _check(load().sora_hip_stream_synchronize(_stream_ptr(None)))
    return out, plan.offsets, [int(v) for v in plan.state[:, 0].cpu().numpy()]


# ---- the 40 MHz HT 2x2 receiver's bricks as stages (include/sora_hip.h, sora_hip_data_symbol_ht40 .. sora_hip_noise_var_ht40)
def data_symbol_ht40(in0, in1, first, nsym, out_first, out0, out1, max_nsym=None, stream=None):
    """2 x 160 -> 2 x 128: frame f's nsym[f] symbols of 160 samples from sample first[f] of in0 / in1 -> their samples 32..159 at symbol out_first[f] of out0 / out1
    (int16 CUDA [symbols * 128, 2])"""
    _check(load().sora_hip_data_symbol_ht40(_dev_ptr(in0), _dev_ptr(in1), _dev_ptr(first), _dev_ptr(nsym), _dev_ptr(out_first), _dev_ptr(out0), _dev_ptr(out1),
                                            first.shape[0], _max_n(nsym, max_nsym), _stream_ptr(stream)))
    return out0, out1


def mimo_est_ht40(ltf0, ltf1, noise_var=None, want_h=True, stream=None):
    """ltf0 / ltf1: int16 CUDA [n, 256, 2] (HT-LTF 1 | HT-LTF 2 of RX chain 0 / 1 after FFT<128>); noise_var: float32 CUDA [n] or None (zero forcing)
    -> (h or None, w) int16 CUDA [n, 4, 128, 2]: the channel matrix and the detection weights x 2^16, entries 00, 01, 10, 11 per bin"""
    import torch
    n = ltf0.shape[0]
    w = torch.empty((n, 4, 128, 2), dtype=torch.int16, device=ltf0.device)
    h = torch.empty_like(w) if want_h else None
    _check(load().sora_hip_mimo_est_ht40(_dev_ptr(ltf0), _dev_ptr(ltf1), _dev_ptr(noise_var) if noise_var is not None else None, _dev_ptr(h) if want_h else None,
                                         _dev_ptr(w), n, _stream_ptr(stream)))
    return h, w


def mimo_comp_ht40(w, y0, y1, frame_index=None, stream=None):
    """w: int16 CUDA [nframes, 4, 128, 2]; y0 / y1: int16 CUDA [nsym, 128, 2]; frame_index: int32 CUDA [nsym] or None -> (x0, x1), the two spatial streams"""
    import torch
    x0 = torch.empty_like(y0); x1 = torch.empty_like(y1)
    _check(load().sora_hip_mimo_comp_ht40(_dev_ptr(w), _dev_ptr(frame_index) if frame_index is not None else None, _dev_ptr(y0), _dev_ptr(y1), _dev_ptr(x0), _dev_ptr(x1),
                                          y0.shape[0], _stream_ptr(stream)))
    return x0, x1


def pilot_track_ht40(x0, x1, first, nsym, state, want_theta=True, stream=None):
    """x0 / x1: int16 CUDA [nsym_total, 128, 2]; first / nsym: int32 CUDA [nframes]; state int16 CUDA [nframes, 24], words 16..23 updated in place
    -> theta int16 CUDA [nsym_total] (word 16 as it stands after each symbol) or None"""
    import torch
    th = torch.zeros(x0.shape[0], dtype=torch.int16, device=x0.device) if want_theta else None
    _check(load().sora_hip_pilot_track_ht40(_dev_ptr(x0), _dev_ptr(x1), _dev_ptr(first), _dev_ptr(nsym), _dev_ptr(state), _dev_ptr(th) if want_theta else None,
                                            state.shape[0], _stream_ptr(stream)))
    return th


def demap_ht40(x, n_bpsc, stream=None):
    """x: int16 CUDA [n, 128, 2] (the detected symbols of one spatial stream) -> uint8 CUDA [n, 108 n_bpsc]"""
    import torch
    out = torch.empty((x.shape[0], 108 * n_bpsc), dtype=torch.uint8, device=x.device)
    _check(load().sora_hip_demap_ht40(_dev_ptr(x), _dev_ptr(out), int(n_bpsc), x.shape[0], _stream_ptr(stream)))
    return out


def deinterleave_ht40(s, n_bpsc, spatial_stream, stream=None):
    """s: uint8 CUDA [n, 108 n_bpsc] of spatial stream 0 or 1 -> de-interleaved, same shape"""
    import torch
    out = torch.empty_like(s)
    _check(load().sora_hip_deinterleave_ht40(_dev_ptr(s), _dev_ptr(out), int(n_bpsc), int(spatial_stream), s.shape[0], _stream_ptr(stream)))
    return out


def stream_join_ht40(s0, s1, n_bpsc, out=None, stream=None):
    """s0 / s1 uint8 CUDA [n, 108 n_bpsc] -> uint8 CUDA [n, 216 n_bpsc], groups of max(n_bpsc / 2, 1) bytes alternating stream 0 / 1"""
    import torch
    n = s0.shape[0]
    if out is None:
        out = torch.empty((n, 216 * n_bpsc), dtype=torch.uint8, device=s0.device)
    _check(load().sora_hip_stream_join_ht40(_dev_ptr(s0), _dev_ptr(s1), _dev_ptr(out), int(n_bpsc), n, _stream_ptr(stream)))
    return out


def downsample_ht40(in0, in1, first, n, m0, out_first, out0, out1, max_n=None, stream=None):
    """the derotating decimator: stream f's kept sample m = raw sample first[f] + 2 m of in0 / in1, negated (saturating) when m0[f] + m is odd, at sample out_first[f] + m of
    out0 / out1; first / n / m0 / out_first int32 CUDA [streams]"""
    _check(load().sora_hip_downsample_ht40(_dev_ptr(in0), _dev_ptr(in1), _dev_ptr(first), _dev_ptr(n), _dev_ptr(m0), _dev_ptr(out_first), _dev_ptr(out0), _dev_ptr(out1),
                                           first.shape[0], _max_n(n, max_n), _stream_ptr(stream)))
    return out0, out1


def noise_var_ht40(lltf0, lltf1, stream=None):
    """lltf0 / lltf1: int16 CUDA [n, 128, 2] (the two L-LTF symbols of chain 0 / 1 after FFT<64>) -> (S int64 CUDA [n], noise_var float32 CUDA [n])"""
    import torch
    n = lltf0.shape[0]
    S = torch.zeros(n, dtype=torch.int64, device=lltf0.device); nv = torch.zeros(n, dtype=torch.float32, device=lltf0.device)
    _check(load().sora_hip_noise_var_ht40(_dev_ptr(lltf0), _dev_ptr(lltf1), _dev_ptr(S), _dev_ptr(nv), n, _stream_ptr(stream)))
    return S, nv


class _GpuHt40Ops(_Gpu11nOps):
    """rx_ht40_stages' bricks on the GPU (the 802.11n ones it shares are _Gpu11nOps'); downsample / noise_var are the front end's two own stages"""
    VOUT = 4352                                                                   # decoded bytes per job: LENGTH <= 4000

    def state(self, rec):
        return self._up(rec, np.int16)

    def downsample(self, iq0, iq1, first, n, m0, out_first, total):
        o0 = self.torch.zeros((max(total, 1), 2), dtype=self.torch.int16, device=self.dev); o1 = self.torch.zeros_like(o0)
        downsample_ht40(iq0, iq1, self._up(first), self._up(n), self._up(m0), self._up(out_first), o0, o1, max_n=int(max(n)))
        return o0[:total], o1[:total]

    def noise_var(self, l0, l1):
        S, nv = noise_var_ht40(l0.reshape(-1, 128, 2), l1.reshape(-1, 128, 2))
        return S.cpu().numpy(), nv.cpu().numpy()

    def data_symbol(self, x0, x1, first, nsym, out_first, total):
        o0 = self.torch.zeros((max(total, 1) * 128, 2), dtype=self.torch.int16, device=self.dev); o1 = self.torch.zeros_like(o0)
        data_symbol_ht40(x0, x1, self._up(first), self._up(nsym), self._up(out_first), o0, o1, max_nsym=int(max(nsym)))
        return o0[:total * 128], o1[:total * 128]

    def fft128(self, x):
        return fft128(x.reshape(-1, 128, 2)).reshape(-1, 2)

    def mimo_est(self, l0, l1, noise_var):
        return mimo_est_ht40(l0.reshape(-1, 256, 2), l1.reshape(-1, 256, 2), self._up(noise_var, np.float32))

    def mimo_comp(self, w, y0, y1, frame_index):
        return mimo_comp_ht40(w, y0.reshape(-1, 128, 2), y1.reshape(-1, 128, 2), self._up(frame_index))

    def pilot_track(self, x0, x1, first, nsym, state):
        return pilot_track_ht40(x0, x1, self._up(first), self._up(nsym), state).cpu().numpy()

    def demap(self, x, nb):
        return demap_ht40(x.reshape(-1, 128, 2), nb)

    def deinterleave(self, s, nb, iss):
        return deinterleave_ht40(s, nb, iss)

    def stream_join(self, s0, s1, nb):
        return stream_join_ht40(s0, s1, nb)

    def viterbi(self, soft, soft_off, nsoft, lens, code_rate):
        ws = self.torch.empty(viterbi11n_workspace_bytes(soft.numel(), len(lens)), dtype=self.torch.uint8, device=self.dev)
        out = viterbi11n_ws(soft, self._up(soft_off), self._up(nsoft), self._up(lens, np.int16), int(code_rate), ws, out_stride=self.VOUT)
        self.torch.cuda.synchronize(self.dev)
        return out.reshape(-1)


def ht40_frame_symbols(d, coding=0):
    """data symbols of the described frame d = (offset, n_bpsc, code_rate, length0, length1, ...) in the given coding: ceil((16 + 8 LENGTH + 6) / N_DBPS), N_DBPS = 108 N_BPSC R
    per stream (sora_ht40_symbols), twice that over the one PSDU of the joint coding (sora_ht40_symbols_joint); 0: a bad descriptor"""
    nb, cr = int(d[1]), int(d[2]) & ~HT40_SHORT_GI                                # (the guard interval does not change N_SYM)
    if nb not in (1, 2, 4, 6) or cr not in (0, 1, 2):
        return 0
    nd = 108 * nb * (1, 2, 3)[cr] // (2, 3, 4)[cr]
    if coding == HT40_CODING_JOINT:
        return (16 + 8 * int(d[3]) + 6 + 2 * nd - 1) // (2 * nd)
    return (16 + 8 * max(int(d[3]), int(d[4])) + 6 + nd - 1) // nd


def rx_ht40_stages(ops, iq0, iq1, frames, coding=0):
    """The data field of described 40 MHz HT two-stream frames (what sora_ht40_process_dev decodes) composed from the stage entry points through `ops` (the GPU's:
    rx_ht40_by_stages; the model's: tests/ht40_stage_model.ModelOps).  frames: [(offset, n_bpsc, code_rate, length0, length1, cfo, noise_var[, id])], the handle's
    descriptors; coding HT40_CODING_PER_STREAM (two PSDUs, two rows per frame) or HT40_CODING_JOINT (length1 = 0, one row).  The host builds the tables; nothing is read back
    between stages but the tracked phase it reports.
      1. freq_comp11n over the two HT-LTF symbols (state {k cfo | 8 cfo | 0}: the brick's own advance keeps the phase n cfo - theta running over the frame) ->
         data_symbol_ht40 -> fft128 -> mimo_est_ht40;
      2. symbol by symbol over the batch, because theta of symbol d rotates symbol d + 1: freq_comp11n -> data_symbol_ht40 -> fft128 -> mimo_comp_ht40 -> pilot_track_ht40;
         a frame that has ended takes part with a count of 0;
      3. over all symbols of a modulation at once: demap_ht40 -> deinterleave_ht40 (-> stream_join_ht40) -> per code rate viterbi11n_ws -> desc11a -> frame_sink11a.
    A descriptor whose code_rate carries HT40_SHORT_GI is a short-GI frame (data symbols of 144 samples, prefix 16), composed from the same stages: in step 2 its
    freq_comp11n runs over 18 bursts at offset + 320 + 144 d, and its data_symbol_ht40 starts 16 samples EARLIER, at offset + 320 + 144 d - 16, so that the stage's samples
    32..159 are exactly the symbol's 128 useful ones (the 16 in front are skipped unread by what follows).  Rows of such a frame carry "short_gi": True.
    -> dict: rows [{frame, stream, error_code, length, crc32, nsym, mpdu}] (frame-major), soft (per frame [stream 0, stream 1] uint8, or the merged bytes in joint coding),
    theta (per frame int16 [nsym + 1]: theta[d] compensates symbol d, the last entry stands after the last symbol), weights and h (ops buffers [frames, 4, 128, 2]), xs (per
    frame int16 [nsym, 2, 128, 2], the detected symbols)."""
    joint = coding == HT40_CODING_JOINT
    nf = len(frames)
    if nf == 0:
        return {"rows": [], "soft": [], "theta": [], "weights": None, "h": None, "xs": []}
    nsym = np.array([ht40_frame_symbols(d, coding) for d in frames], np.int64)
    for d, n in zip(frames, nsym):
        if n == 0 or d[3] > 4000 or d[4] > 4000 or (joint and d[4] != 0) or not (d[6] >= 0):
            raise ValueError("rx_ht40_stages: bad frame descriptor (n_bpsc 1/2/4/6, code_rate 0..2, PSDU <= 4000 bytes, noise_var >= 0; joint coding: length1 = 0)")
    off = np.array([int(d[0]) for d in frames], np.int64); nbp = np.array([int(d[1]) for d in frames], np.int64)
    cfo = np.array([int(d[5]) for d in frames], np.int64)
    sgi = np.array([(int(d[2]) & HT40_SHORT_GI) != 0 for d in frames], bool)
    pitch = np.where(sgi, 144, 160); lead = np.where(sgi, 16, 0)                  # a short symbol: 18 bursts; the stage's 160-sample window starts 16 early
    rate = [int(d[2]) & ~HT40_SHORT_GI for d in frames]
    u32 = lambda a: np.asarray(a, np.int64).astype(np.uint32).view(np.int32)
    i16 = lambda a: ((np.asarray(a, np.int64) + 32768) & 0xFFFF) - 32768
    rec = np.zeros((nf, 24), np.int16)
    rec[:, :8] = i16(cfo[:, None] * np.arange(8)[None, :]); rec[:, 8:16] = i16(8 * cfo)[:, None]
    st = ops.state(rec)
    # ---- 1. the two HT-LTF symbols
    c0, c1 = ops.freq_comp(iq0, iq1, u32(off), u32(np.full(nf, 40)), st)
    y0, y1 = ops.data_symbol(c0, c1, u32(off), u32(np.full(nf, 2)), u32(2 * np.arange(nf)), 2 * nf)
    h, w = ops.mimo_est(ops.fft128(y0), ops.fft128(y1), np.array([d[6] for d in frames], np.float32))
    # ---- 2. the data symbols
    theta = [[0] for _ in range(nf)]
    xs0 = [[] for _ in range(nf)]; xs1 = [[] for _ in range(nf)]
    for d in range(int(nsym.max())):
        al = np.nonzero(nsym > d)[0]
        nbur = np.zeros(nf, np.int64); nbur[al] = pitch[al] // 8
        c0, c1 = ops.freq_comp(iq0, iq1, u32(off + 320 + pitch * d), u32(nbur), st)
        y0, y1 = ops.data_symbol(c0, c1, u32(off[al] + 320 + pitch[al] * d - lead[al]), u32(np.ones(len(al))), u32(np.arange(len(al))), len(al))
        x0, x1 = ops.mimo_comp(w, ops.fft128(y0), ops.fft128(y1), u32(al))
        pf = np.zeros(nf, np.int64); pn = np.zeros(nf, np.int64); pf[al] = np.arange(len(al)); pn[al] = 1
        th = ops.pilot_track(x0, x1, u32(pf), u32(pn), st)
        for i, f in enumerate(al):
            theta[f].append(int(th[i])); xs0[f].append(x0[i]); xs1[f].append(x1[i])
    # ---- 3. per modulation: every symbol at once
    soft = [None] * nf
    for b in (1, 2, 4, 6):
        fs = [f for f in range(nf) if nbp[f] == b]
        if not fs:
            continue
        d0 = ops.deinterleave(ops.demap(ops.concat([x for f in fs for x in xs0[f]]), b), b, 0)
        d1 = ops.deinterleave(ops.demap(ops.concat([x for f in fs for x in xs1[f]]), b), b, 1)
        jn = ops.stream_join(d0, d1, b) if joint else None
        at = 0
        for f in fs:
            n = int(nsym[f])
            soft[f] = jn[at:at + n].reshape(-1) if joint else [d0[at:at + n].reshape(-1), d1[at:at + n].reshape(-1)]
            at += n
    jobs = [(f, 0) for f in range(nf)] if joint else [(f, s) for f in range(nf) for s in range(2)]
    rows = [None] * len(jobs)
    for cr in (0, 1, 2):
        js = [j for j, (f, s) in enumerate(jobs) if rate[f] == cr]
        if not js:
            continue
        parts = [soft[jobs[j][0]] if joint else soft[jobs[j][0]][jobs[j][1]] for j in js]
        nsoft = np.array([int(p.shape[0]) for p in parts], np.int64)
        lens = np.array([int(frames[jobs[j][0]][3 + jobs[j][1]]) for j in js], np.int64)
        dec = ops.viterbi(ops.concat(parts), u32(np.concatenate([[0], np.cumsum(nsoft)])[:-1]), u32(nsoft), lens, cr)
        boff = 4096 * np.arange(len(js))
        by = ops.desc(dec, u32(ops.VOUT * np.arange(len(js))), u32(lens), u32(boff), 4096 * len(js))
        srec = ops.frame_sink(by, u32(boff), u32(lens)); hb = ops.host(by)
        for i, j in enumerate(js):
            f, s = jobs[j]
            rows[j] = {"frame": f, "stream": s, "error_code": int(srec[i, 0]), "length": int(lens[i]), "crc32": int(srec[i, 1]), "nsym": int(nsym[f]),
                       "short_gi": bool(sgi[f]), "mpdu": hb[boff[i]:boff[i] + lens[i]].tobytes()}
    xs = [np.stack([np.stack([ops.host(a).reshape(128, 2), ops.host(b).reshape(128, 2)]) for a, b in zip(xs0[f], xs1[f])]) for f in range(nf)]
    return {"rows": rows, "soft": [ops.host(s) if joint else [ops.host(s[0]), ops.host(s[1])] for s in soft], "theta": [np.array(t, np.int16) for t in theta],
            "weights": w, "h": h, "xs": xs}


def rx_ht40_by_stages(d_iq0, d_iq1, frames, coding=0):
    """sora_ht40_process_dev's result for the described frames through the stage entry points alone (rx_ht40_stages with the GPU's bricks): d_iq0 / d_iq1 int16 CUDA
    [samples, 2].  A DEMONSTRATION and a test vehicle, not a fast path: five launches per OFDM symbol of the longest frame and every intermediate through HBM, against the
    handle's one kernel.  The fast path is RxHt40."""
    return rx_ht40_stages(_GpuHt40Ops(d_iq0.device), d_iq0, d_iq1, frames, coding)


def ht40_sig_gate(rec):
    """The 40 MHz front end's gate on the decoded bits of one sora_hip_sig_decode11n record (words 9..11): T11nSigParser's checks in front of its own gate (L-SIG reserved
    bits, parity, rate code, LENGTH field; HT-SIG CRC-8), then 8 <= MCS <= 14 && CBW 40 && 4 <= LENGTH <= 4000 -> None (SORA_E_PLCP_HEADER_FAIL) or (mcs, ht_length)"""
    sig = int(rec[9]) & 0xFFFFFF; ht = int(rec[10]) | (int(rec[11]) << 32)
    if (sig & 0xFC0010) or (bin(sig).count("1") & 1) or (sig & 0xF) < 8 or ((sig >> 5) & 0xFFF) * 2 > 1500:
        return None
    crc = 0xFF
    for b in range(34):
        crc ^= (ht >> b) & 1
        crc = (crc >> 1) ^ 0xE0 if crc & 1 else crc >> 1
    if ((~crc) & 0xFF) != ((ht >> 34) & 0x3FFF):
        return None
    mcs = ht & 0x7F; cbw40 = (ht >> 7) & 1; length = (ht >> 8) & 0xFFFF
    if mcs < 8 or mcs > 14 or not cbw40 or length < 4 or length > 4000:
        return None
    return mcs, length


def rx_ht40_front_stages(ops, iq0, iq1, descs, coding=0):
    """The front end of the 40 MHz HT receiver (what sora_ht40_process_captures_dev does in front of its data field) up to the FIRST event of every capture, composed from
    stages through `ops`: downsample_ht40 -> the 802.11n stages along rx11n_stages' walk (cca11n | cfo_est11n -> freq_comp11n -> fft64 -> siso_est11n | freq_comp11n ->
    data_symbol11n -> fft64 -> siso_comp11n -> sig_demap11n -> sig_decode11n) -> ht40_sig_gate on the host -> noise_var_ht40 on the L-LTF's transforms.
    descs: [(first sample, samples)] over the two chains at 40 MHz, whole 28-sample source calls at offsets that are multiples of 4.
    -> per capture None (no detection; the capture ends inside the header; a sound header whose frame runs past the capture: no event, as the handle has it) or a
    sora_ht40_found-shaped dict a20, mcs, ht_len, nsym, cfo, noise_var (numpy float32), S, end_sample, error_code, and, for a recorded frame, "descriptor": the sora_ht40_frame
    by k_ht40_plan's rule (offset = capture + 2 a20 + 160, cfo / 2 truncated toward zero, each stream LENGTH bytes; joint coding: one PSDU).
    Carrier-sense time-outs re-arm at the burst that raises them, as in rx11n_stages.  A demonstration and a test vehicle, not a fast path."""
    nc = len(descs)
    if nc == 0:
        return []
    off = np.array([int(d[0]) for d in descs], np.int64); ns = np.array([int(d[1]) for d in descs], np.int64)
    if (ns % 28).any() or (off % 4).any():
        raise ValueError("rx_ht40_front_stages: a capture is whole 28-sample source calls at an offset that is a multiple of 4")
    u32 = lambda a: np.asarray(a, np.int64).astype(np.uint32).view(np.int32)
    n20 = ns // 2
    first = np.concatenate([[0], np.cumsum(n20)])[:-1]
    x0, x1 = ops.downsample(iq0, iq1, u32(off), u32(n20), u32(np.zeros(nc)), u32(first), int(n20.sum()))
    nb = n20 // 4
    st, used = ops.cca(x0, x1, u32(first), u32(nb), cca11n_states(nc), CCA11N_REARM)
    s0 = first + 4 * used.astype(np.int64); left = 4 * (nb - used.astype(np.int64))
    events = [None] * nc
    live = np.array([c for c in range(nc) if st[c, 0] == 1 and left[c] >= 368], np.int64)
    if len(live) == 0:
        return events
    s0 = s0[live]; nl = len(live)
    vfo = ops.cfo_est(ops.take(x0, s0, 128), ops.take(x1, s0, 128))
    cfo = np.array(ops.host(vfo)).reshape(nl, 24)[:, 1].astype(np.int64)          # vfo_delta_i[1] = the estimate, before TFreqComp_11n advances the record
    c0, c1 = ops.freq_comp(x0, x1, u32(s0), u32(np.full(nl, 16)), vfo)
    l0, l1 = ops.fft64(ops.take(c0, s0, 128)), ops.fft64(ops.take(c1, s0, 128))
    ch = ops.siso_est(l0, l1)
    S, nv = ops.noise_var(l0, l1)
    c0, c1 = ops.freq_comp(x0, x1, u32(s0 + 128), u32(np.full(nl, 30)), vfo)
    y0, y1 = ops.data_symbol11n(c0, c1, u32(s0 + 128), u32(np.full(nl, 3)), u32(3 * np.arange(nl)), 3 * nl)
    rec = ops.sig_decode(ops.sig_demap(ops.siso_comp_mrc(ch, ops.fft64(y0), ops.fft64(y1), u32(np.repeat(np.arange(nl), 3)))))
    call = lambda kept, c: int(min(-(-2 * kept // 28) * 28, ns[c]))             # the source call (28 raw samples) that brings the kept sample in front of position `kept`
    for j, c in enumerate(live):
        a20 = int(s0[j] + 368 - first[c])
        ev = {"a20": a20, "mcs": 0, "ht_len": 0, "nsym": 0, "cfo": int(cfo[j]), "noise_var": np.float32(nv[j]), "S": int(S[j]), "end_sample": call(a20, c),
              "error_code": E_PLCP_HEADER_FAIL}
        g = ht40_sig_gate(rec[j])
        if g is not None:
            mcs, length = g
            nbp = {8: 1, 9: 2, 10: 2, 11: 4, 12: 4, 13: 6, 14: 6}[mcs]; cr = 2 if mcs in (10, 12, 14) else 1 if mcs == 13 else 0
            nsym = ht40_frame_symbols((0, nbp, cr, length, 0 if coding == HT40_CODING_JOINT else length), coding)
            end = a20 + 80 * (nsym + 3)                                          # HT-STF, two HT-LTFs and the data symbols at the 20 MHz rate
            if 2 * end > ns[c]:
                continue                                                        # the frame runs past the capture: no event
            h = int(cfo[j]); half = -((-h) // 2) if h < 0 else h // 2
            ev.update({"mcs": mcs, "ht_len": length, "nsym": nsym, "end_sample": call(end, c), "error_code": 0,
                       "descriptor": (int(off[c]) + 2 * a20 + 160, nbp, cr, length, 0 if coding == HT40_CODING_JOINT else length, half, float(nv[j]), int(c))})
        events[c] = ev
    return events


def rx_ht40_front_by_stages(d_iq0, d_iq1, descs, coding=0):
    """The first sora_ht40_found record of every capture of a batch of two-chain 40 MHz captures, and the descriptor k_ht40_plan makes of it, through the stage entry points
    alone (rx_ht40_front_stages with the GPU's bricks).  A DEMONSTRATION and a test vehicle, not a fast path; the first event only, and no end-of-capture flush."""
    return rx_ht40_front_stages(_GpuHt40Ops(d_iq0.device), d_iq0, d_iq1, descs, coding)


_GpuHt40Ops.data_symbol11n = _Gpu11nOps.data_symbol
