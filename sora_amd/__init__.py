"""sora_amd -- MI355X-native 802.11a receive PHY behind Sora's BRICK operator shapes.

The product is sora_amd/lib/libsora_hip.so (hand-written HIP for gfx950, C ABI in include/sora_hip.h);
this package is the thin Python binding used by the tests and bench.py.  There is no CPU compute path.
"""
from .capi import (Rx, Rx11b, Rx11n, RxHt40, ht40_symbols, HostResults, ROW_DTYPE, ROW_TRUNCATED, ROW_SHORT_PREAMBLE, SoraError, device_count, load, lib_path, fft64, fft128, lts11a, symfront11a,
    pilot_track11a, pilot11a, set_share_window_us, freq_comp11a, equalize11a, phase_comp11a, demap11a, deinterleave11a, demap11n, deinterleave11n, mimo_est11n, mimo_comp11n,
    cfo_est11n, freq_comp11n, pilot_track11n, siso_est11n, siso_comp11n, sig_demap11n, sig_decode11n, viterbi11a, viterbi11a_ws, viterbi11a_workspace_bytes,  # noqa: F401
                   viterbi11n_ws, viterbi11n_workspace_bytes, viterbi_window_stats, viterbi56_11n, CR_56,
                   ingest, ingest_count, scramble11a, conv_encode11a, interleave11a, map11a, add_pilot11a, ifftx11a, upsample40to44, pack16to8, preamble11a,
                   mod11a_by_stages, Mod11aStages, mod11a_fields, CR_12, CR_23, CR_34,
                   stream_parse11n, interleave11n, map11n, sig_map11n, add_pilot11n, ifft_only11n, csd11n, add_gi11n, preamble11n,
                   mod11n_by_stages, Mod11nStages, mod11n_fields,
                   dc_remove11b, energy_detect11b, symtiming11b, barker_sync11b, despread11b, sfd_sync11b, dbpsk_demap11b, dqpsk_demap11b, cck5p5_decode11b,
                   cck11_decode11b, desc741_11b, plcp_parse11b, frame_sink11b, rx11b_by_stages, rx11b_stages, state11b_reset, STATE11B_WORDS,
                   cca11n, cca11n_states, data_symbol11n, stream_join11n, desc11a, frame_sink11a, rx11n_by_stages, rx11n_stages, CCA11N_WORDS, CCA11N_REARM,
                   dc_remove11a, dc_estimate11a, cca11a, carrier_sense11a, data_symbol11a, viterbi_sig11a, plcp_parse11a, cca11a_states, dcest11a_states, cs11a_states,
                   cca11a_reset, cs11a_record_words, rx11a_stages, rx11a_by_stages, CCA11A_WORDS, DCEST11A_WORDS, CS11A_WORDS, CCA11A_STOP_ON_TIMEOUT,
                   ppdu11b, sc741_11b, dbpsk_spread11b, dqpsk_spread11b, cck5_encode11b, cck11_encode11b, pulse_shape11b, mod11b_by_stages, Mod11bStages,
                   tx11a, tx11a_samples, tx11n, tx11n_samples, tx_ht40, tx_ht40_samples, tx11b, tx11b_samples, INGEST_RXBLOCK, INGEST_RAW14, INGEST_44TO40, INGEST_DECIMATE2,
                   ht40_symbols_joint, HT40_CODING_PER_STREAM, HT40_CODING_JOINT, tx_ht40_joint, tx_ht40_joint_samples,
                   stream_parse_ht40, interleave_ht40, interleave_ht40_stream, map_ht40, sig_map_ht40, add_pilot_ht40, ifft_ht40, add_gi_ht40, preamble_ht40,
                   mod_ht40_by_stages, ModHt40Stages, mod_ht40_fields,
                   tx_ht40_gi_samples, tx_ht40_joint_gi_samples, HT40_SHORT_GI, ROW_SHORT_GI, HT40_GUARD_LONG, HT40_GUARD_SIGNALLED,
                   data_symbol_ht40, mimo_est_ht40, mimo_comp_ht40, pilot_track_ht40, demap_ht40, deinterleave_ht40, stream_join_ht40, downsample_ht40, noise_var_ht40,
                   rx_ht40_stages, rx_ht40_by_stages, ht40_frame_symbols, rx_ht40_front_stages, rx_ht40_front_by_stages, ht40_sig_gate,
                   E_FRAME_OK, E_CRC32_FAIL, E_PLCP_HEADER_FAIL, TRELLIS_WINDOWED, table_names, table_pin, table_digest, table_read)
