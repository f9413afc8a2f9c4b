/* sora_hip.h -- C ABI of the MI355X-native 802.11a receive PHY (libsora_hip.so).
 *
 * The reference (microsoft/Sora) has no runtime FFI: its "operator API" is the compile-time BRICK
 * protocol (kernel/brick/inc/brick.h:151-475 -- Process / Reset / Flush on typed burst ports, shared
 * state in context facades, errors as bool + CF_Error::error_code).  This header is the boundary a
 * maintainer binds instead: every entry point below names the reference brick(s) it replaces.  Bricks
 * fire per 4/28/64 samples, a kernel launch per Process() is impossible, so the ports are kept but the
 * BURST is a batch (BRICK allows any BURST/NSTREAM: brick.h:182-238).
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns a BK_ERROR_* / E_ERROR_* compatible code
 *     (kernel/brick/inc/dspcomm.h:22-31, kernel/bb/Brick11/src/ieee80211facade.hpp:10-19)
 *   - pointers named d_* are DEVICE (HBM) pointers, h_* are host pointers; the caller owns every buffer
 *   - calls on one handle must be serialised by the caller, different handles are independent and may be used from
 *     different threads (no hidden globals, unlike the reference's BB11aDemodCtx,
 *     kernel/bb/demod11/fb11ademod_config.hpp:123; the per-device look-up tables of the stage entry points are
 *     created once under a lock)
 *   - the library never falls back to a CPU path: without a usable HIP device every compute call
 *     returns SORA_ERR_NO_DEVICE.
 */
#ifndef SORA_HIP_H
#define SORA_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)     /* libsora_hip.so is built with -fvisibility=hidden: what this header declares is what it exports */
#endif

/* 3 (round 5).  Against 2: (i) behaviour that round 4 changed under the old number: a call that has been delivered (sora_rx_deliver_async) AND waited for
 * (sora_rx_wait / _wait_any; the same for the rx11b / rx11n / ht40 handles) is RELEASED -- its pipeline is the first to be reused, so its ticket is valid for `depth`
 * further calls only if the host has not both delivered and waited for it; sora_rx_set_fused(1) answers SORA_E_NOT_SUPPORTED (k_decode has since been removed);
 * sora_rx11b_set_single_pass defaults to 2 (automatic); sora_ht40_deliver_async needs max_rows >= 2 x captures x max_frames.  (ii) new this round, all additive:
 * SORA_TRELLIS_WINDOWED and sora_rx_window_stats, sora_rx_set_front / sora_rx_front, sora_hip_table_*, sora_hip_freq_comp11a / _equalize11a / _phase_comp11a,
 * and the automatic choices of sora_rx_set_trellis / sora_rx_set_front (results are identical whichever kernels run).  INTEGRATION.md section 1 lists them. */
/* 4 (round 6).  Against 3: no row is ever delivered with SORA_E_INTERNAL_TIMEOUT (see sora_rx_set_front, form 4); new, additive: sora_rx_set_pipe_wait_us, sora_rx_pipe_stats,
 * sora_hip_pilot11a, sora_rx_bind_mpdu, sora_rx11n_trellis, sora_rx11n_window_stats, sora_rx_call_front, sora_rx_set_ordered, sora_hip_set_share_window_us, SORA_TRELLIS_WINDOWED and
 * the automatic choice for sora_rx11n_set_trellis.
 * Additive since: the 802.11a modulation graph's bricks as stages -- sora_hip_scramble11a, _conv_encode11a, _interleave11a, _map11a, _add_pilot11a (_from), _ifftx11a,
 * _upsample40to44, _pack16to8, _preamble11a; the 802.11n modulation graphs' -- sora_hip_stream_parse11n, _interleave11n, _map11n, _sig_map11n, _add_pilot11n,
 * _ifft_only11n, _csd11n, _add_gi11n, _preamble11n; the 802.11b modulation graph's -- sora_hip_ppdu11b, _sc741_11b, _dbpsk_spread11b, _dqpsk_spread11b, _cck5_encode11b,
 * _cck11_encode11b, _pulse_shape11b (sora_mod11b_state, sora_shaper11b_state); the 40 MHz HT receiver's bricks -- sora_hip_data_symbol_ht40, _mimo_est_ht40, _mimo_comp_ht40,
 * _pilot_track_ht40, _demap_ht40, _deinterleave_ht40, _stream_join_ht40, _downsample_ht40, _noise_var_ht40; the bricks that complete the 802.11n receive graph -- sora_hip_cca11n
 * (sora_cca11n_state), _data_symbol11n, _stream_join11n, and the tail it shares with the 802.11a graph, sora_hip_desc11a, _frame_sink11a (sora_sink11a_rec); the front end
 * of the 802.11a receive graph -- sora_hip_dc_remove11a, _dc_estimate11a (sora_dcest11a_state), _cca11a (sora_cca11a_state), _carrier_sense11a (sora_cs11a_state),
 * _data_symbol11a, _viterbi_sig11a, _plcp_parse11a (sora_plcp11a_rec); the 40 MHz HT modulation graph's bricks -- sora_hip_stream_parse_ht40, _interleave_ht40,
 * _interleave_ht40_stream, _map_ht40, _sig_map_ht40, _add_pilot_ht40, _ifft_ht40, _add_gi_ht40, _preamble_ht40; the K=7 decoder at code rate 5/6 as a stage --
 * sora_hip_viterbi56_11n (SORA_CR_56), and MCS 15 on the 40 MHz pair -- sora_ht40_set_mcs_max, sora_hip_tx_ht40_mcs, _joint_mcs and their _samples. */
#define SORA_HIP_ABI_VERSION 4

/* COMPLEX16: kernel/core/inc/complex.h */
typedef struct { int16_t re, im; } sora_complex16;

/* status codes (values of the reference where one exists) */
#define SORA_OK                  0           /* BK_ERROR_SUCCESS / E_ERROR_SUCCESS */
#define SORA_E_FRAME_OK          0x00000001  /* E_ERROR_FRAME_OK */
#define SORA_E_PARAMETER         ((int)0x80000001)
#define SORA_E_PLCP_HEADER_FAIL  ((int)0x80000005)
#define SORA_E_CRC32_FAIL        ((int)0x80000006)
/* retired: ABI 3 reported a frame with it when a bounded wait inside k_pipe expired; since ABI 4 no row carries it (the call is made again on the device) */
#define SORA_E_INTERNAL_TIMEOUT  ((int)0x8000F001)
#define SORA_ERR_FAILED          ((int)0x8000FFFF)  /* BK_ERROR_FAILED */
#define SORA_ERR_HARDWARE_FAILED ((int)0x8000FFFE)  /* BK_ERROR_HARDWARE_FAILED: a HIP call failed */
#define SORA_ERR_INVALID_PARAM   (-1)               /* BK_ERROR_INVALID_PARAM */
#define SORA_ERR_NO_DEVICE       (-5)
#define SORA_ERR_CAPACITY        (-6)               /* a caller-provided buffer or a configured limit is too small */

/* code rates: kernel/bb/Brick11/src/ieee80211const.h:14-20 */
enum { SORA_CR_12 = 0, SORA_CR_23 = 1, SORA_CR_34 = 2 };
/* Rate 5/6 (BB11nGetCodingRateFromMcsIndex names CR_56; the reference has no encoder or decoder for it, so the definition is this library's, held to an integer
 * model): per 5 input bits the coded bits sent are A1 B1 A2 B3 A4 B5 (IEEE 802.11n-2009) -- the reference's 3/4 pattern A1 B1 A2 B3 continued by A4 B5.  A puncture
 * group is 6 soft values and 5 trellis steps of kinds (A,B) (A) (B) (A) (B).  It is taken by sora_hip_viterbi56_11n, by the descriptors of a 40 MHz receive
 * handle whose gate is 15 (sora_ht40_set_mcs_max) and by sora_ht40_symbols, and it is what sora_hip_tx_ht40_mcs sends at MCS 15; every other entry point that takes a code
 * rate accepts SORA_CR_12 / _23 / _34 and answers 3 with SORA_ERR_INVALID_PARAM. */
enum { SORA_CR_56 = 3 };

/* ------------------------------------------------------------------------------------------------
 * Whole-path receiver = the demod graph CreateDemodGraph11a_40M (kernel/bb/demod11/fb11ademod_config.hpp:
 * 168-233) driven by RxThread (kernel/bb/demod11/fb11a_demod.cpp:29-81), over a BATCH of independent captures.
 * ------------------------------------------------------------------------------------------------ */
typedef struct sora_rx sora_rx_t;

typedef struct {
    uint32_t struct_size;           /* sizeof(sora_rx_cfg) */
    int32_t  device;                /* HIP device ordinal */
    uint32_t sample_rate_mhz;       /* 40: dump rate, TDownSample2 first (samples.hpp:9-47); 20: the even samples;
                                     * 44: CreateDemodGraph11a_44M (fb11ademod_config.hpp:236-300) -- iq is the 40 MHz stream
                                     * sora_hip_ingest(SORA_INGEST_44TO40) makes of a 44 MHz dump; as in that graph, the
                                     * resampler's queued samples survive the reset after a frame (TDownSample44_40 has no
                                     * Reset/Flush).  Positions are 20 MHz-rate samples of the resampled stream. */
    uint32_t max_captures;          /* captures per sora_rx_process call */
    uint64_t max_total_samples;     /* sum of capture lengths per call (input-rate samples) */
    uint32_t max_frames_per_capture;/* frame-table rows per capture */
    uint32_t cca_pwr_threshold;     /* CF_11CCA::cca_pwr_threshold; 0 -> 1000*1000 (fb11ademod_config.hpp:107) */
} sora_rx_cfg;

typedef struct {                    /* one capture = one TMemSamples source (brick/inc/memsource.hpp:16-114) */
    uint64_t offset;                /* first sample, in samples, from the iq base pointer; multiple of 4 (16-byte aligned) */
    uint32_t nsamples;              /* input-rate samples */
    uint32_t capture_id;            /* echoed into the results */
} sora_capture_desc;

typedef struct {                    /* one row per frame the reference's RxThread would have reported */
    uint32_t capture_id;
    uint32_t start_sample;          /* 20 MHz-rate index (in the capture) of the first sample given to T11aLTS */
    uint32_t end_sample;            /* one past the last 20 MHz-rate sample of the frame */
    uint32_t error_code;            /* SORA_E_FRAME_OK / SORA_E_CRC32_FAIL / SORA_E_PLCP_HEADER_FAIL */
    uint32_t rate_kbps;             /* CF_11aRxVector::data_rate_kbps */
    uint16_t length;                /* CF_11aRxVector::frame_length (MPDU incl. FCS) */
    uint16_t nsym;                  /* data symbols */
    uint32_t crc32;                 /* FCS found in the frame (CF_11aRxVector::crc32) */
    int16_t  cfo_est;               /* CF_CFOffset::CFO_est (FP_RAD per sample) */
    uint16_t flags;                 /* SORA_ROW_TRUNCATED on the LAST row of a capture that held more frames than
                                     * max_frames_per_capture: the reference's RxThread reports every frame, the frames after
                                     * this one were found but have no row */
    uint32_t mpdu_offset;           /* byte offset of the MPDU in the mpdu buffer */
} sora_frame_result;

#define SORA_ROW_TRUNCATED 1u
#define SORA_ROW_SHORT_PREAMBLE 2u       /* 802.11b rows: the frame came behind the short preamble (sora_rx11b_set_preamble) */
#define SORA_ROW_SHORT_GI 4u             /* 40 MHz HT rows: the frame had the short guard interval (SORA_HT40_SHORT_GI, sora_ht40_set_guard) */

/* create/destroy the graph: CreateDemodGraph11a_40M + BB11aDemodCtx.Init  /  IReferenceCounting::Release */
int  sora_rx_create(const sora_rx_cfg* cfg, sora_rx_t** out);
void sora_rx_destroy(sora_rx_t* rx);
/* ISource::Reset / ISource::Flush (brick.h:343-353): Reset forgets all per-call state; Flush waits for the stream */
int  sora_rx_reset(sora_rx_t* rx);
int  sora_rx_flush(sora_rx_t* rx);
/* The stream every kernel of this handle is launched on (a hipStream_t), for event timing by the caller. */
void* sora_rx_stream(sora_rx_t* rx);

/* ISource::Process over a batch: enqueue the whole receive path for `ncaps` captures whose samples are
 * resident in HBM (d_iq).  Asynchronous; results become available after sora_rx_flush / sora_rx_results. */
int  sora_rx_process_dev(sora_rx_t* rx, const sora_complex16* d_iq, const sora_capture_desc* h_caps, size_t ncaps);
/* Same with a host buffer (copied to HBM first; the PCIe time is then part of the call). */
int  sora_rx_process(sora_rx_t* rx, const sora_complex16* h_iq, size_t total_samples, const sora_capture_desc* h_caps, size_t ncaps);
/* LoadSoraDumpFile -> graph -> MPDU buffer as ONE stream-ordered path (brickutil.h:20-58 in front of fb11a_demod.cpp:88-120): the raw dump
 * bytes in host memory (page-locked for a copy that overlaps the other calls in flight: sora_hip_host_alloc) go up to the call's
 * pipeline, sora_hip_ingest (flags SORA_INGEST_*: RX_BLOCK de-framing, 14 -> 16 bit, 44 -> 40 MHz, TDownSample2) runs on the device and
 * the receive chain decodes the result; no host wait anywhere.  The capture descriptors address the INGESTED sample stream (its length is
 * sora_hip_ingest_count(dump_bytes, flags), at the handle's sample_rate_mhz).  The host buffer must stay untouched until the call has
 * completed (sora_rx_wait).  Ticket, results and delivery as for sora_rx_process_dev. */
int  sora_rx_process_dump(sora_rx_t* rx, const void* h_dump, size_t dump_bytes, unsigned ingest_flags, const sora_capture_desc* h_caps, size_t ncaps);
/* Stream continuation (the live-source case: TRxStream hands the graph an endless stream, brick/inc/rxstream.hpp:34-66, and the graph's
 * state -- the DC estimate, which integrates for ever (dc.hpp:92-166), the carrier-sense windows and counters (cca.hpp:126-158) -- carries
 * over from one read to the next).  With sora_rx_set_stream_mode(rx, 1) capture k of a process call CONTINUES capture k of the call before it:
 *   - after a call, sora_rx_stream_consumed(rx, ticket, h, n) gives, per capture, the RESUME POINT: the number of input-rate samples of that
 *     capture that are final (a position where a burst boundary of the graph falls on a source-call boundary while it is in plain carrier
 *     sense; 0 if the capture holds none).  Every frame the call reported ends in front of it; a frame that was still running when the
 *     capture ended lies behind it and has NOT been reported;
 *   - the host builds the next call's capture k from the stream FROM THAT POINT on: the unconsumed tail of what it submitted plus whatever
 *     has arrived since (each capture still a whole number of 28-sample source bursts; 14 at 20 MHz).  The library starts it with the state
 *     the graph had at the resume point, so the rows of all the calls together (positions are relative to their own capture: add the
 *     stream position of its first sample) are exactly the events the graph reports on the uncut stream -- tests/test_gpu_stream.py holds a
 *     40 MHz stream cut at arbitrary 28-sample boundaries to the compiled reference graph's events on the whole;
 *   - calls of a handle in stream mode run one after the other (a process call first waits for the one before it: it needs its records);
 *     throughput comes from many streams (captures) per call.  sora_rx_reset, and switching the mode, start every stream afresh;
 *   - sample_rate_mhz = 44 (CreateDemodGraph11a_44M): TDownSample44_40 is empty only on its period, 308 source samples in, 280 out.  So a
 *     resume point is also a multiple of 280 resampled samples (140 at 20 MHz), and `used` is one.  The host keeps the 44 MHz source,
 *     resumes it at used * 11 / 10 (a multiple of 308 = 11 RX_BLOCKs) and ingests each piece on its own (sora_hip_ingest with
 *     SORA_INGEST_44TO40, or sora_rx_process_dump); a piece may end at any RX_BLOCK.  Several pieces in one dump: each starts a multiple of
 *     11 RX_BLOCKs in (zero blocks as padding), capture offset (first block / 11) * 280, length sora_hip_ingest_count(piece bytes, flags).
 *     A frame is reported by the first call whose capture holds a resume point behind it.  That point may lie up to 280 resampled samples
 *     behind the frame's end (more if another frame follows at once), so a capture can end before it; the frame is then withheld: no row,
 *     and no MPDU byte written, also not into an array bound with sora_rx_bind_mpdu (its data field is decoded all the same, and again by
 *     the call that reports it).  So every row still ends in front of `used`, and the rows of all calls are the uncut stream's events
 *     (tests/test_gpu_stream44.py).
 *   Returns the previous mode; a negative argument only queries. */
int  sora_rx_set_stream_mode(sora_rx_t* rx, int enable);
int  sora_rx_stream_consumed(sora_rx_t* rx, int ticket, uint32_t* h_consumed, size_t ncaps);
/* Diagnostic: a copy of the continuation record of capture `capture` (index into the call's captures) as the handle's most recent call left it,
 * after that call has completed: *n_words = 64 words, the graph's carrier-sense state at the capture's last resume point (words 0-15 sample_his in
 * time order, already >> 2; 16-19 / 20-23 / 24-27 the auto-correlation (re, im) and energy windows, oldest first; 28-30 their sums; 31 sense_count;
 * 32 high_count; 33 peak_corr; 34 peak_index; 35 the DC estimator's countdown; 36-37 its sums; 38-39 the DC estimate; 40 the resume point; 41 a
 * magic word once a record exists; 42 the frames reported in front of the point; the rest 0).  tests/test_gpu_scan_sense.py holds every word to the
 * reference graph's restatement.  SORA_ERR_INVALID_PARAM when stream mode is off or the call has no such capture, SORA_ERR_CAPACITY (with *n_words
 * set) when cap_words is too small.  Read-only. */
int  sora_rx_stream_record_of(sora_rx_t* rx, int ticket, uint32_t capture, uint32_t* h_words, size_t cap_words, size_t* n_words);

/* TBB11aFrameSink's frame buffer + CF_Error per frame: copies results of the last process call to the host.
 * h_mpdu may be NULL (descriptors only).  *nout = rows written. Frames appear in (capture, time) order.
 * mpdu_offset indexes h_mpdu and counts the bytes COPIED in front of the row: with h_mpdu NULL every row's offset is 0, and a row behind one whose MPDU did
 * not fit carries the offset that one carries.  A buffer that is short gives SORA_ERR_CAPACITY with what fits delivered: max_out short -- the first max_out
 * rows, *nout = max_out; mpdu_cap short -- every row, each MPDU that would reach past mpdu_cap skipped (a later, shorter one that fits is still copied).  The
 * same holds for *_results / *_results_of of the 802.11b and 802.11n handles (tests/deliver_model.py states it, tests/test_gpu_deliver.py holds the handles to it). */
int  sora_rx_results(sora_rx_t* rx, sora_frame_result* h_out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap);

/* Tickets.  With several calls in flight (sora_rx_set_depth) every process call has a TICKET, a positive number that
 * identifies the call until its pipeline is reused: by the `depth`-th process call after it, or earlier once the call is
 * RELEASED -- its delivery was enqueued (sora_rx_deliver_async) and it has been waited for (sora_rx_wait / sora_rx_wait_any),
 * so that everything it produced is in the caller's memory.
 * What fb11a_demod.cpp:37-71 does per frame -- look at the result, hand the MPDU to the MAC -- is done per call with these:
 *   sora_rx_ticket          ticket of the most recent process call (0: none yet)
 *   sora_rx_wait            block until that call has finished (its kernels and any sora_rx_deliver_async copies)
 *   sora_rx_results_of      sora_rx_results for that call
 *   sora_rx_results_dev_of  sora_rx_results_dev for that call
 *   sora_rx_stream_of       the HIP stream that call runs on
 *   sora_rx_deliver_async   enqueue, behind the call's kernels and without blocking the host, the delivery of its results
 *                           into host memory: the dense rows (capture, time order; at most max_rows are copied), their
 *                           number, and -- h_mpdu != NULL -- the MPDU array (row.mpdu_offset indexes it; mpdu_bytes must be
 *                           at least sora_rx_mpdu_bytes(rx, ticket); a smaller h_mpdu is refused, SORA_ERR_CAPACITY, before anything is enqueued).
 *                           The array has 32 bytes per symbol slot, a capture's nsamples / 80 + 1 slots (20 MHz-rate samples) behind those of the
 *                           captures before it, and a frame's MPDU starts at the slot of its SIGNAL symbol, (start_sample + 144) / 80 of its
 *                           capture; the offsets are the same whether or not h_mpdu is given.  The buffers should be page-locked
 *                           (sora_hip_host_alloc) so that the copies overlap later calls; they are valid after sora_rx_wait.
 *   sora_rx_wait_any        block until SOME call whose delivery has been enqueued has finished, and return its ticket (the oldest
 *                           one if several have).  Calls in flight overtake one another (their streams sit on different dispatch
 *                           priorities and share the chip); a host that always waits for its oldest ticket leaves the pipelines of the
 *                           calls that finished first idle until the slowest one is through (measured: a third of every pipeline's
 *                           time, profiles/r04_t_own_timeline.txt).  RxThread's loop (fb11a_demod.cpp:37-71) with this call:
 *                               process_dev -> deliver_async -> [depth calls in flight?] wait_any -> hand that call's MPDUs to the MAC.
 *                           The next process call reuses a released pipeline first.  SORA_ERR_FAILED if no such call is in flight.
 * A stale ticket gives SORA_ERR_INVALID_PARAM. */
int    sora_rx_ticket(sora_rx_t* rx);
int    sora_rx_wait(sora_rx_t* rx, int ticket);
int    sora_rx_wait_any(sora_rx_t* rx, int* ticket);
int    sora_rx_results_of(sora_rx_t* rx, int ticket, sora_frame_result* h_out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap);
void*  sora_rx_stream_of(sora_rx_t* rx, int ticket);
size_t sora_rx_mpdu_bytes(sora_rx_t* rx, int ticket);
int    sora_rx_deliver_async(sora_rx_t* rx, int ticket, sora_frame_result* h_rows, size_t max_rows, uint32_t* h_nrows, uint8_t* h_mpdu, size_t mpdu_bytes);
/* A lone call's delivery without the copy behind it (round 6, ABI 4).  sora_rx_bind_mpdu names, for the NEXT process call of the handle only, a page-locked array from
 * sora_hip_host_alloc of at least that call's sora_rx_mpdu_bytes() (SORA_ERR_CAPACITY from the process call otherwise; the array's geometry is the device array's: 32 bytes per
 * symbol slot): the call's frame sink then writes every MPDU there as well, straight over PCIe while the frames are being finished, and sora_rx_deliver_async(ticket, ..) with
 * the SAME h_mpdu copies rows and count only.  The bytes are valid when the ticket has been waited for; words of the array that no frame of the call owns are left as they were.
 * For a host that keeps ONE or TWO calls in flight (the MPDU copy is a lone 4096-frame call's 0.22 ms tail); with many calls in flight their copies overlap anyway and
 * waves that wait on PCIe writes hold compute units the other calls' kernels want (measured in round 3): do not bind there.  h_mpdu = NULL cancels a binding not yet used. */
int    sora_rx_bind_mpdu(sora_rx_t* rx, uint8_t* h_mpdu, size_t mpdu_bytes);
/* Per-kernel timing with HIP events recorded on the streams the kernels run on (SoraStopwatch / MACStopwatch analogue,
 * kernel/bb/demod11/MACStopwatch.h:84-128).  With profiling enabled every process call brackets each kernel launch
 * with events; sora_rx_kernel_times waits for the calls in flight and returns, in launch order, the MEAN duration (ms)
 * of each kernel over all process calls since profiling was (re-)enabled.  Calls in flight on different pipelines
 * share the CUs, so these are the durations the kernels really had, not what each would take alone. */
int  sora_rx_set_profiling(sora_rx_t* rx, int enable);
int  sora_rx_kernel_times(sora_rx_t* rx, float* h_ms, size_t cap, size_t* nout);
const char* sora_rx_kernel_name(size_t index);

/* Consecutive process calls rotate over `depth` internal pipelines (own stream, own intermediate arrays), so the
 * latency-bound front end of one call overlaps the trellis kernel of the call before it -- what the reference gets from
 * running ViterbiThread beside RxThread (fb11a_demod.cpp:117-120).  Default 8, 1 = strictly
 * one call at a time, at most 16.  (The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues, 4 by default, one of them
 * the null stream's: a host that wants more than three calls to actually run side by side sets that variable, as bench.py does -- 16; measured:
 * the step time of the benchmark batch stops improving at eight calls in flight on twelve or more queues.)  Returns the previous value; depth <= 0 only queries.  sora_rx_results / _results_dev /
 * _stream refer to the MOST RECENT process call, the *_of forms to the call whose ticket is given; sora_rx_flush waits for
 * every call in flight; an input buffer must stay untouched until the call that reads it has finished (as with any
 * asynchronous call). */
int  sora_rx_set_depth(sora_rx_t* rx, int depth);

/* Two trellis kernels decode the soft stream of the split data-field path, bit for bit the same T11aViterbi (viterbi.hpp:103-237):
 *   64  k_viterbi    the 64 states of a frame pair in the 64 lanes of a wave: two frames per wave, the most waves -- the faster
 *                    one while few frames are in flight (one 4096-frame call: 2048 waves for 1024 SIMDs);
 *   16  k_viterbi16  a frame pair in 16 lanes x 4 registers, eight frames per wave: half the vector instructions per frame and
 *                    no cross-row exchanges, but a quarter of the waves -- the faster one once several calls are in flight.
 *   SORA_TRELLIS_WINDOWED (1)  k_viterbi16w (round 5): the frame's 256-bit trace-back windows (viterbi.hpp:196-214) decoded side by side, each run from
 *                    all-equal metrics a warm-up ahead of its first window and PROVEN afterwards -- its metric vector at the preceding normalisation
 *                    point must equal its predecessor's there (k_win_redo); a frame with a mismatch is decoded again serially by the same kernel.  Bit-exact by
 *                    construction; the kernel for few frames in flight (one capture, one lone call), where a frame per wave-slot leaves the chip idle.
 *   0   (default)    chosen by the library from the handle's capacity in flight: k_viterbi16 when depth x max_captures >= 32768
 *                    (eight 4096-capture calls, two 16384-capture calls), the window-parallel form below that.
 * Returns the previous setting; a negative argument only queries. */
#define SORA_TRELLIS_WINDOWED 1
int  sora_rx_set_trellis(sora_rx_t* rx, int lanes_per_pair);
int  sora_rx_trellis(sora_rx_t* rx);            /* the kernel the next process call will use: 64, 16 or SORA_TRELLIS_WINDOWED (resolves the automatic choice) */
/* The window-parallel trellis's proof record since the handle was created: out[0] unit boundaries compared, out[1] boundaries whose vectors differed,
 * out[2] frames decoded again by the serial kernel because of that, out[3] units.  Waits for the handle's calls in flight. */
int  sora_rx_window_stats(sora_rx_t* rx, unsigned long long out[4]);
/* Three forms of the symbol chain T11aDataSymbol .. T11aDeinterleave (fb11ademod_config.hpp:200-222) write the same soft stream:
 *   1   k_frame      one wave per frame, four symbols per pass, the pilot tracker's loop-carried chain in the same wave: the cheaper one when the chip is full of frames;
 *   3   k_sym_front -> k_track_lds -> k_sym_back   per symbol slot in front of and behind the tracker (TFreqCompensation, TFFT64, TChannelEqualization | TPhaseCompensate's
 *                    rotation, T11aDemap, T11aDeinterleave), and the tracker's chain (freqoffset.hpp:28-30, pilot.hpp:166-233) alone, four lanes per frame, with its
 *                    three look-up tables folded into LDS: a frame's symbols spread over the chip -- the one for few, long frames (fsample-6: 465 symbols);
 *   4   k_pipe       form 3 AND the window-parallel trellis as ONE launch whose workgroups hand symbols on as the tracker passes them (the reference's demod || Viterbi
 *                    overlap, fb11a_demod.cpp:109-112, inside a frame): the one for a handful of frames (a single capture).  (Its trellis units run two per wave in k_viterbi's
 *                    64-lane layout while the handle's calls in flight are few enough for that many workgroups -- a lone capture with up to three calls in flight --, eight per wave
 *                    otherwise.)  Used only with the window-parallel trellis and
 *                    where every workgroup of the handle's calls in flight is resident at once (at most three quarters of the device's compute units: 192 on an MI355X); otherwise a request
 *                    for 4 runs as 3.  Its hand-offs
 *                    are bounded waits (sora_rx_set_pipe_wait_us): should one expire -- another process or other GPU work holds the compute units its workgroups need -- the
 *                    launch's finishing kernel makes the call's data field again with form 1's code and the serial trellis, so the call still delivers the reference's rows
 *                    (never an error code of this library's own), and the handle keeps to form 3 for its next 64 calls (sora_rx_pipe_stats counts both);
 *                    it is the form for an otherwise idle chip -- each of its workgroups takes a whole CU's LDS, so beside a chip kept full by other handles its launch waits for CUs
 *                    to drain and form 3 is the faster one (measured: 3.3 against 1.3 ms median beside eight 4096-capture calls in flight; tools/pipe_under_load.py);
 *   0   (default)    chosen by the library: 4 while depth x max_captures x max_frames_per_capture <= 16 (and it fits, and no batch-sized handle of this process has used
 *                    the device within the last 20 ms), 3 up to 512, else 1.
 * Returns the previous setting; a negative argument only queries. */
int  sora_rx_set_front(sora_rx_t* rx, int kernels);
int  sora_rx_front(sora_rx_t* rx);              /* 1, 3 or 4: what the next process call will use */
/* The automatic choice looks at the clock (has another, batch-sized handle of the process taken a call on this device within the share window?), so sora_rx_front is a
 * forecast.  What a call WAS launched with is latched at its process call: sora_rx_call_front (ticket 0 = the most recent call) answers 1, 3 or 4 for as long as the handle
 * holds the ticket.  sora_hip_set_share_window_us sets the window for the whole process (default 20000; 0 = other handles are never looked at) and returns the old value. */
int  sora_rx_call_front(sora_rx_t* rx, int ticket);
/* Completion in submission order (round 6; 0 / 1, returns the previous setting; default 0).  Calls in flight share the chip and, left alone, finish together: a host that hands a
 * batch over in pieces to get its first frames early gets nothing.  With 1 the trellis kernel of a call starts behind the trellis kernel of the call submitted before it: the
 * calls complete one after the other, a call's front kernels still run beside the trellis of the one before it and its delivery beside the trellis of the one after it.  For the
 * host that wants frames as early as possible (the reference's per-frame hand-over, fb11a_demod.cpp:37-71); the throughput-oriented loop (eight unordered calls) is faster per
 * sample.  Results are identical either way.  (An ordered call is launched kernel by kernel, not as a recorded hipGraph.) */
int  sora_rx_set_ordered(sora_rx_t* rx, int on);
uint32_t sora_hip_set_share_window_us(uint32_t us);
/* k_pipe's safety net.  The bound of every wait inside its launch, in microseconds (default 20000; 0 = a wait that is not satisfied at first look gives up: every call
 * then takes the redo path -- what tests/test_gpu_pipe.py does to prove that path delivers the reference's rows).  Returns the previous bound; a negative argument only queries. */
int  sora_rx_set_pipe_wait_us(sora_rx_t* rx, long long us);
/* out[0] = calls since the handle was created whose data field was made again because a wait inside k_pipe gave up, out[1] = times the handle then switched itself to
 * form 3 for 64 calls.  Waits for the handle's calls in flight. */
int  sora_rx_pipe_stats(sora_rx_t* rx, unsigned long long out[2]);
/* Identical consecutive calls (same buffer, same capture set) may be replayed as ONE hipGraph launch instead of a chain of
 * kernel launches: 1 = on, 0 = off (default).  Returns the previous setting; a negative argument only queries. */
int  sora_rx_set_graph(sora_rx_t* rx, int enable);

/* The data field (T11aDataSymbol .. T11aViterbi) is decoded by k_frame (symbol chain, soft values to HBM one pre-scaled byte each)
 * followed by k_viterbi16 / k_viterbi (sora_rx_set_trellis).  Rounds 2-3 also shipped k_decode -- both in one kernel, symbol waves
 * feeding trellis waves through a ring in LDS the way the reference's RxThread feeds its ViterbiThread through TThreadSeparator
 * (stdbrick.hpp:89-248) -- which lost to the split form at every depth (0.80 against 0.46 ms per step, BENCH_r03), left the library
 * in round 4 and has since been REMOVED.  The two entry points stay in the ABI: sora_rx_set_fused(rx, 1) returns SORA_E_NOT_SUPPORTED
 * and changes nothing; enable = 0 and the query (enable < 0) return 0.  sora_rx_kernel_name_fused(i) still names the kernels of the
 * removed chain ("" = slot not used). */
int  sora_rx_set_fused(sora_rx_t* rx, int enable);
const char* sora_rx_kernel_name_fused(size_t index);

/* Device-side views of the last call's outputs (valid until the next process/reset/destroy). */
int  sora_rx_results_dev(sora_rx_t* rx, const sora_frame_result** d_rows, const uint32_t** d_nrows, const uint8_t** d_mpdu);
int  sora_rx_results_dev_of(sora_rx_t* rx, int ticket, const sora_frame_result** d_rows, const uint32_t** d_nrows, const uint8_t** d_mpdu);

/* ------------------------------------------------------------------------------------------------
 * Per-stage entry points with the brick port shapes, batched (n = number of bursts).  All pointers are
 * device pointers; `stream` is a hipStream_t (NULL = default stream).  Each can sit behind a BRICK-shaped
 * adapter (include/sora_brick.hpp) where the SSE brick sits today.
 *
 * Every stage entry point of this header -- this block and the stage blocks below, sora_hip_<brick>(..., size_t count, void* stream) -- checks its arguments in one
 * order: a null pointer that is not optional is refused by name (SORA_ERR_INVALID_PARAM); a count of 0 returns SORA_OK (nothing to launch, with or without a
 * device); no device gives SORA_ERR_NO_DEVICE; a count of 2^31 or more gives SORA_ERR_CAPACITY (the kernels index with 32 bits: split the batch).  The checks
 * particular to one entry (n_bpsc, a flag, alignment, its own limits) follow; only sora_hip_stream_join11n and the sora_hip_*_ht40 stages refuse a bad n_bpsc or
 * spatial_stream earlier, before the count is looked at.
 * ------------------------------------------------------------------------------------------------ */
/* TFFT64  (Brick11/src/fft.hpp:108-135 -> core/inc/fft_r4dif.h FFT<64>): IPORT COMPLEX16x64 -> OPORT COMPLEX16x64 */
int sora_hip_fft64(const sora_complex16* d_in, sora_complex16* d_out, size_t n, void* stream);
/* FFT<128> (core/inc/fft_r4dif.h: 4 x 32, 8-point terminal stage; used by the reference's oversampled TX and the
 * shape a 40 MHz HT receiver needs): IPORT COMPLEX16x128 -> OPORT COMPLEX16x128 */
int sora_hip_fft128(const sora_complex16* d_in, sora_complex16* d_out, size_t n, void* stream);
/* T11aLTS (channel_11a.hpp:33-230): IPORT COMPLEX16 x 144 -> the context facades it fills:
 * CF_CFOffset::CFO_est, CF_FreqCompensate::Coeffs[16 vcs], CF_Channel_11a::ChannelCoeffs[16 vcs] */
typedef struct { int16_t cfo_est; int16_t reserved; sora_complex16 freq[64]; sora_complex16 chan[64]; } sora_lts11a_ctx;
int sora_hip_lts11a(const sora_complex16* d_in, sora_lts11a_ctx* d_ctx, size_t n, void* stream);
/* T11aDataSymbol -> TFreqCompensation -> TFFT64 -> TChannelEqualization (PHY_11a.hpp:361-430, channel_11a.hpp:532-653):
 * IPORT COMPLEX16 x 80 -> OPORT COMPLEX16 x 64; symbol i uses d_ctx[d_ctx_index[i]] (d_ctx_index NULL: d_ctx[0]) */
int sora_hip_symfront11a(const sora_complex16* d_in, const sora_lts11a_ctx* d_ctx, const uint32_t* d_ctx_index, sora_complex16* d_eq, size_t n, void* stream);
/* The three one-multiply bricks of the symbol chain on their own (the receive path fuses them; here each can replace its SSE brick alone), IPORT COMPLEX16 x 64 ->
 * OPORT COMPLEX16 x 64, symbol i with the coefficients of d_ctx[d_ctx_index[i]] (index NULL: d_ctx[0]):
 *   TFreqCompensation     (channel_11a.hpp:614-653)  out = ((in >> 1) x CF_FreqCompensate::Coeffs) >> 15.  The brick also leaves in >> 1 in its input queue; the
 *                                                   queue belongs to the caller here and is not written.
 *   TChannelEqualization  (channel_11a.hpp:534-604)  out = (in x CF_Channel_11a::ChannelCoeffs) >> 8, bins 28 .. 35 zero
 *   TPhaseCompensate      (freqoffset.hpp:16-66)     out = (in x CF_PhaseCompensate::CompCoeffs) >> 15 -- sora_track11a_state::comp of d_state[d_state_index[i]] */
int sora_hip_freq_comp11a(const sora_complex16* d_in, const sora_lts11a_ctx* d_ctx, const uint32_t* d_ctx_index, sora_complex16* d_out, size_t n, void* stream);
int sora_hip_equalize11a(const sora_complex16* d_in, const sora_lts11a_ctx* d_ctx, const uint32_t* d_ctx_index, sora_complex16* d_out, size_t n, void* stream);
/* TPhaseCompensate + TPilotTrack (freqoffset.hpp:14-66, pilot.hpp:121-269) over the symbols of n frames, in order:
 * frame f owns symbols d_first[f] .. d_first[f]+d_nsym[f]-1 of d_eq; d_state[f] = CF_PhaseCompensate + CF_PilotTrack,
 * read at entry and written back.  Bins 0 and 27..37 of the output are not defined by the reference and are written 0. */
typedef struct { int16_t cfo_comp, sfo_comp, cfo_tracker, sfo_tracker; uint32_t symbol_count; sora_complex16 comp[64]; } sora_track11a_state;
int sora_hip_pilot_track11a(const sora_complex16* d_eq, const uint32_t* d_first, const uint32_t* d_nsym, sora_track11a_state* d_state,
                            sora_complex16* d_out, size_t nframes, void* stream);
int sora_hip_phase_comp11a(const sora_complex16* d_in, const sora_track11a_state* d_state, const uint32_t* d_state_index, sora_complex16* d_out, size_t n, void* stream);
/* TPilotTrack alone (pilot.hpp:121-269): the same frame tables, d_in = TPhaseCompensate's output (what sora_hip_phase_comp11a wrote for the symbol with the state as it
 * was); rotates the symbol by the pilots' mean phase and slope and advances d_state (the trackers, CFO_comp / SFO_comp, symbol_count, CompCoeffs for the NEXT symbol).
 * The brick that replaces TPilotTrack where TPhaseCompensate stays the reference's (or sora_hip_phase_comp11a's): new in ABI 4. */
int sora_hip_pilot11a(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_nsym, sora_track11a_state* d_state,
                      sora_complex16* d_out, size_t nframes, void* stream);
/* T11aDemap<N_BPSC>::Filter (demapper11a.hpp:10-79): IPORT COMPLEX16x64 -> OPORT uchar x 48*n_bpsc */
int sora_hip_demap11a(const sora_complex16* d_in, uint8_t* d_soft, int n_bpsc, size_t n, void* stream);
/* T11aDeinterleave{BPSK,QPSK,QAM16,QAM64} (deinterleaver.hpp): IPORT uchar x N_CBPS -> OPORT uchar x N_CBPS */
int sora_hip_deinterleave11a(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, size_t n, void* stream);
/* T11aViterbi<5000*8,48,256,24>::Filter (viterbi.hpp:103-237) over n frames: frame i reads nsoft[i] soft values at
 * d_soft + soft_off[i] and writes frame_len[i]+2 decoded bytes at d_out + out_off[i]. */
int sora_hip_viterbi11a(const uint8_t* d_soft, const uint32_t* d_soft_off, const uint32_t* d_nsoft,
                        const uint16_t* d_frame_len, int code_rate, uint8_t* d_out, const uint32_t* d_out_off,
                        size_t n, void* stream);
/* (What stands behind the decoder in the 802.11a graph as in the 802.11n one, T11aDesc -> TBB11aFrameSink, is the stage pair sora_hip_desc11a / sora_hip_frame_sink11a,
 * declared with the 802.11n receive stages below: it reads exactly the frame_len[i] + 2 bytes per frame that this stage writes.) */
/* The same brick for a caller that streams bursts through it (a BRICK adapter calls once per burst): no allocation, no host
 * wait, everything in stream order.  soft_span_bytes = the extent of the caller's soft buffer that the n jobs address
 * (max over i of soft_off[i] + nsoft[i]; the jobs' ranges must not overlap -- any offsets, any order, any nsoft >= 24: a
 * job with less than one OFDM symbol of soft values is not a frame); d_workspace = 16-byte aligned device memory of
 * at least sora_hip_viterbi11a_workspace_bytes(soft_span_bytes, n), owned by the caller and free for reuse once the call's
 * work on `stream` has completed.  (sora_hip_viterbi11a is this entry point over a grow-only workspace the library caches
 * per device; it reads the extent back from the device and waits for the stream before it returns.) */
size_t sora_hip_viterbi11a_workspace_bytes(size_t soft_span_bytes, size_t n);
int sora_hip_viterbi11a_ws(const uint8_t* d_soft, size_t soft_span_bytes, const uint32_t* d_soft_off, const uint32_t* d_nsoft,
                           const uint16_t* d_frame_len, int code_rate, uint8_t* d_out, const uint32_t* d_out_off,
                           size_t n, void* d_workspace, size_t workspace_bytes, int lanes_per_pair, void* stream);
/* lanes_per_pair: which trellis kernel decodes (identical results): 64 (or 0) = k_viterbi, 16 = k_viterbi16, SORA_TRELLIS_WINDOWED =
 * k_viterbi16w + k_win_redo (see sora_rx_set_trellis).  The window-parallel form cuts the n jobs into units by the receive path's own plan, so the
 * batch size decides the units' geometry: one job gives units of one window, a few thousand units of several windows, 16384 or more one unit per job. */
/* T11aViterbi<5000*8,312,192,36>, the 802.11n graph's decoder (fb11ndemod_config.hpp:199), as the same stage: one BYTE per soft value, of which
 * only the low three bits are read (VitJob::soft_bits = 8).  lanes_per_pair: 64 (or 0) = k_viterbi11n, 16 = k_viterbi16_11n, SORA_TRELLIS_WINDOWED =
 * k_viterbi16w_11n + k_win_redo_11n.  The workspace holds a copy of the caller's soft_span_bytes. */
size_t sora_hip_viterbi11n_workspace_bytes(size_t soft_span_bytes, size_t n);
int sora_hip_viterbi11n_ws(const uint8_t* d_soft, size_t soft_span_bytes, const uint32_t* d_soft_off, const uint32_t* d_nsoft,
                           const uint16_t* d_frame_len, int code_rate, uint8_t* d_out, const uint32_t* d_out_off,
                           size_t n, void* d_workspace, size_t workspace_bytes, int lanes_per_pair, void* stream);
/* The proof record of the last SORA_TRELLIS_WINDOWED call of sora_hip_viterbi11a_ws / sora_hip_viterbi11n_ws on this workspace, in
 * sora_rx_window_stats's order: out[0] unit boundaries compared, out[1] boundaries whose vectors differed, out[2] jobs decoded again serially
 * because of that, out[3] units.  Waits for `stream` (the stream of that call).  Calls with another lanes_per_pair leave the record as it was. */
int sora_hip_viterbi_window_stats(const void* d_workspace, unsigned long long out[4], void* stream);
/* The same decoder at code rate 5/6 (SORA_CR_56), a kernel of its own (k_viterbi56_11n): T11aViterbi<.., 192, 36>::Process with a fourth branch and ONE rule changed.
 *   - Per puncture group p[0..5]: ACS(A,B)(p0,p1) ACS(A)(p2) ACS(B)(p3) ACS(A)(p4) ACS(B)(p5), then trellis_index += 5, p += 6.
 *   - The metrics are normalised after every step whose index is a multiple of 8, also inside a group.  (The reference's rule, (trellis_index & 7) == 0 after a group,
 *     would fire every 40 steps -- up to 8 x 84 units of growth in an 8-bit wrapping metric, which decodes nothing; every 8 steps is rate 1/2's cadence with less growth,
 *     at most 140 units against 224.)
 *   - The trace-back schedule is examined after every group with the other rates' expressions: a frame's last trace-back at the first group end with trellis_index >=
 *     8 length + 22 (look = the excess, 0..4); else, from trellis_index >= ob + 192 + 36 + 6 on, a window of 192 bits with look = 36 + remain, remain =
 *     (trellis_index - (ob + 234)) % 8 (0..4).  Metric initialisation, tie-breaks, the arg-min key and the 6-bit prefix are unchanged.
 *   - Soft values short of a whole group at the end of a stream are not decoded; a stream that ends in front of its frame's last trace-back yields the whole windows
 *     it holds and nothing else.
 * tests/cxx/viterbi56_model.c states all of it as a program, and the kernel is held to it bit for bit.  One BYTE per soft value, of which only the low three bits are
 * read (what sora_ht40_soft_of returns); job i reads d_nsoft[i] bytes at d_soft + d_soft_off[i] (any alignment) and writes d_frame_len[i] + 2 decoded bytes at d_out +
 * d_out_off[i].  Consecutive jobs (2k, 2k + 1) share a wave.  soft_span_bytes = the extent of d_soft: no byte at or behind d_soft + soft_span_bytes is ever read,
 * whatever the offsets say, so the stage needs no workspace and no slack behind the last stream; 0 is SORA_ERR_INVALID_PARAM, 2^32 or more SORA_ERR_CAPACITY.  No
 * allocation and no host wait.  Not offered: the sixteen-lane and window-parallel forms, a rate 5/6 encoder stage (sora_hip_conv_encode11a keeps refusing rate 3),
 * BRICK adapters. */
int sora_hip_viterbi56_11n(const uint8_t* d_soft, size_t soft_span_bytes, const uint32_t* d_soft_off, const uint32_t* d_nsoft, const uint16_t* d_frame_len,
                           uint8_t* d_out, const uint32_t* d_out_off, size_t n, void* stream);

/* Capture ingest in front of the receive graph, one streaming pass on the device:
 *   SORA_INGEST_RXBLOCK    the input is a Sora dump: 128-byte RX_BLOCKs = 16-byte descriptor + 28 COMPLEX16
 *                          (LoadSoraDumpFile, kernel/brick/inc/brickutil.h:20-58; kernel/core/inc/_rx_manager.h:96-137)
 *   SORA_INGEST_RAW14      samples are 14-bit two's complement, zero-extended: x = (int16)(raw << 2)
 *   SORA_INGEST_44TO40     TDownSample44_40 / Down44to40 (Brick11/src/sampling.hpp:35-66, 44MTo40M.hpp:62-123)
 *   SORA_INGEST_DECIMATE2  TDownSample2 (Brick11/src/samples.hpp:9-47): keep the even samples (40 -> 20 MHz)
 * applied in that order.  d_raw: the dump bytes (or, without RXBLOCK, a COMPLEX16 stream) in device memory;
 * sora_hip_ingest_count gives the number of samples the call writes (a function of the size and flags only). */
#define SORA_INGEST_RXBLOCK   1u
#define SORA_INGEST_RAW14     2u
#define SORA_INGEST_44TO40    4u
#define SORA_INGEST_DECIMATE2 8u
size_t sora_hip_ingest_count(size_t raw_bytes, unsigned flags);
int sora_hip_ingest(const void* d_raw, size_t raw_bytes, unsigned flags, sora_complex16* d_out, size_t out_capacity,
                    size_t* n_out, void* stream);

/* 802.11a transmitter: the modulation graph CreateModGraph11a_* of the reference
 * (kernel/bb/demod11/fb11amod_config.hpp:74-110: TBB11aSrc -> T11aSc -> TConvEncode_* -> T11aInterleave* -> TMap11a* ->
 * T11aAddPilot -> TIFFTx -> TPackSample16to8) plus the preamble (Brick11/src/preamble11a.hpp:19-140), a batch of frames per
 * call.  Frame f: MPDU WITHOUT FCS (the FCS is appended, PHY_11a.hpp:160-170) of d_len[f] bytes at d_mpdu + d_off[f], data
 * rate d_rate_kbps[f] (6000..54000), scrambler seed d_seed[f] (the reference harness uses 0xFF, fb11amod_config.hpp:53);
 * writes sora_hip_tx11a_samples(len, rate) COMPLEX8 samples (int8 re, int8 im) at 40 MHz -- what `demod11 -m` writes --
 * at sample d_out_off[f] of d_out.  A frame with an unknown rate must not be submitted (sora_hip_tx11a_samples = 0). */
size_t sora_hip_tx11a_samples(uint32_t mpdu_len_nofcs, uint32_t rate_kbps);
int sora_hip_tx11a(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps,
                   const uint8_t* d_seed, size_t nframes, int8_t* d_out, const uint64_t* d_out_off, void* stream);

/* The same transmitter at a Sora radio's own 44 MHz: CreateModGraph11a_44M + CreatePreamble11a_44M (fb11amod_config.hpp), the graphs
 * the reference's live applications send with (kernel/bb/umxsdrbrick/dot11main.cpp:222-223, umxsdra/dot11main.cpp:201-202,
 * umxsniffer/dot11main.cpp:212-213, kernel/bb/demod11/fb11a_mod.cpp:39-40).  They are the 40 MHz graphs with TUpsample40MTo44M
 * (Brick11/src/sampling.hpp:8-32, 40MTo44M.hpp) between TIFFTx (or TTS11aSrc) and TPackSample16to8.  The brick turns each 160-sample
 * block x of 16-bit samples into 176 samples y and carries nothing from block to block; for I and Q apart, m = 0..15:
 *     mh(a, c)  = (a * c + 16384) >> 15                                           (_mm_mulhrs_epi16)
 *     S(k)      = floor(k * 32767 / 11)                                           (k = 1..10)
 *     y[11m]    = mh(x[10m], 32767)
 *     y[11m+r]  = int16(mh(x[10m+r-1], S(r)) + mh(x[10m+r], S(11-r)))             (r = 1..10)
 * and only then are the samples saturated to 8 bits: upsampling the 40 MHz COMPLEX8 stream instead differs wherever that stream
 * touches a rail.  y[175] needs x[160], which the reference loads from behind its input block (40MTo44M.hpp:112).  The preamble source
 * hands its 640 samples on as one burst, so its blocks 0..2 see the next block's first sample there, and so do they here.  Its block 3,
 * the SIGNAL symbol and every data symbol read whatever memory follows the pin queue's buffer -- an accident of the build's layout, not
 * arithmetic -- and here x[160] = 0 for them: sample 176 j + 175 of a frame, j >= 3, is the closed form with x[160] = 0.
 * A frame is sora_hip_tx11a44_samples(len, rate) = 11/10 of sora_hip_tx11a_samples(len, rate) samples (0 where that is 0), d_out_off
 * counts 44 MHz samples; every other rule, error code and null check is sora_hip_tx11a's. */
size_t sora_hip_tx11a44_samples(uint32_t mpdu_len_nofcs, uint32_t rate_kbps);
int sora_hip_tx11a44(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps,
                     const uint8_t* d_seed, size_t nframes, int8_t* d_out, const uint64_t* d_out_off, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The bricks of the 802.11a modulation graph as stage entry points: what CreateModGraph11a_40M / _44M and CreatePreamble11a_40M / _44M
 * (kernel/bb/demod11/fb11amod_config.hpp:74-110) are built from, each with the port format of the brick it replaces -- bits packed in bytes,
 * LSB first, exactly as the brick's pins carry them -- so that a host can replace ONE brick, or compose the graphs from stages:
 *     preamble -> [upsample40to44] -> pack16to8
 *     scramble -> conv_encode -> interleave -> map -> add_pilot -> ifftx -> [upsample40to44] -> pack16to8
 * The conventions are those of the stage entry points above: device pointers, stream order, no allocation, no host wait; a null pointer or a symbol
 * buffer that is not 16-byte aligned gives SORA_ERR_INVALID_PARAM, no device SORA_ERR_NO_DEVICE, a count of 0 is SORA_OK and launches nothing.
 * (The byte streams of the scrambler and the encoder lie at the caller's offsets and need no alignment.)  DESIGN.md section 7, f2b.
 * ------------------------------------------------------------------------------------------------ */
/* T11aSc (Brick11/src/scramble.hpp:170-261): IPORT uchar x 1 -> OPORT uchar x 1.  Frame f owns d_len[f] bytes at d_off[f] of both buffers (in place is
 * fine).  The register starts at d_seed[f] -- the brick after Reset: all 8 bits are stored, each byte takes lut[reg >> 1].  Every byte is DO_SCRAMBLE except
 * byte d_tail[f] where d_tail != NULL and d_tail[f] < d_len[f]: TAIL_SCRAMBLE, (b ^ reg) & 0xC0, the register advancing all the same.  NO_SCRAMBLE is not
 * calling the stage.  max_len: a bound on every d_len[f] that the host knows (it sizes the grid; bytes of a frame at or behind it are not written). */
int sora_hip_scramble11a(const uint8_t* d_in, uint8_t* d_out, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_tail, const uint8_t* d_seed,
                         size_t nframes, size_t max_len, void* stream);
/* TConvEncode_12 / _23 / _34 (conv_enc.hpp:18-330): IPORT uchar x 1 / 2 / 3 -> OPORT uchar x 2 / 3 / 4, code_rate = SORA_CR_12 / _23 / _34.  Frame f reads
 * d_len[f] bytes at d_in + d_in_off[f], the register 0 at its first byte, and writes its whole bursts' output at d_out + d_out_off[f] in the bricks' bit order
 * and puncturing (A B; A B A; A B A B').  Input bytes behind the last whole burst produce nothing (the brick leaves them queued); nothing behind the frame's
 * output is written.  max_len as above, below 128 MiB. */
int sora_hip_conv_encode11a(const uint8_t* d_in, const uint32_t* d_in_off, const uint32_t* d_len, int code_rate, uint8_t* d_out, const uint32_t* d_out_off,
                            size_t nframes, size_t max_len, void* stream);
/* T11aInterleave{BPSK,QPSK,QAM16,QAM64} (interleave.hpp:16-114; N_COL = 16, I_SS = 1): IPORT uchar x 6 n_bpsc -> OPORT uchar x 6 n_bpsc per symbol */
int sora_hip_interleave11a(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, size_t nsym, void* stream);
/* TMap11a{BPSK,QPSK,QAM16,QAM64}<MOD> (mapper11a.hpp:8-300): IPORT uchar x 6 n_bpsc -> OPORT COMPLEX16 x 48 per symbol.  mod = the brick's MOD template argument
 * (1 .. 32767); 0 = the 802.11a default for n_bpsc: 10720, (short)(10720 / 1.414), / 3.162, / 6.481.  (The 802.11n graph instantiates the same bricks with
 * 30339, 21453, 9594 and 4681.) */
int sora_hip_map11a(const uint8_t* d_in, sora_complex16* d_out, int n_bpsc, int mod, size_t nsym, void* stream);
/* T11aAddPilot<BPSK_MOD> (pilot.hpp:30-118): IPORT COMPLEX16 x 48 -> OPORT COMPLEX16 x 64 per symbol: the data carriers placed, the four pilots, every other bin 0.
 * Frame f owns symbols d_first[f] .. d_first[f] + d_nsym[f] - 1 (sora_hip_pilot_track11a's frame tables).  The symbol at position j of its frame takes
 * PilotSgn[127] for j = 0 and PilotSgn[(j - 1) mod 127] otherwise: the brick's m_PilotIndex starts at 127 and wraps at 127 (j = 0 is the SIGNAL symbol of a real
 * frame).  bpsk_mod = 0 means 10720.  _from: table entry f is the part of a frame that begins at position d_pos0[f] (what a brick adapter that streams bursts
 * of one frame needs); d_pos0 NULL = 0 everywhere = sora_hip_add_pilot11a. */
int sora_hip_add_pilot11a(const sora_complex16* d_in, sora_complex16* d_out, const uint32_t* d_first, const uint32_t* d_nsym, size_t nframes, int bpsk_mod,
                          void* stream);
int sora_hip_add_pilot11a_from(const sora_complex16* d_in, sora_complex16* d_out, const uint32_t* d_first, const uint32_t* d_nsym, const uint32_t* d_pos0,
                               size_t nframes, int bpsk_mod, void* stream);
/* TIFFTx (fft.hpp:7-61): IPORT COMPLEX16 x 64 -> OPORT COMPLEX16 x 160 per symbol.  Bins 0..31 and 32..63 go to bins 0..31 and 96..127 of the reference's fixed-point
 * IFFT<128>; then >> 4, the last 32 samples copied to the front as the guard interval, and samples 0, 1, 158, 159 halved. */
int sora_hip_ifftx11a(const sora_complex16* d_in, sora_complex16* d_out, size_t nsym, void* stream);
/* TUpsample40MTo44M (sampling.hpp:8-32, 40MTo44M.hpp): IPORT COMPLEX16 x 160 -> OPORT COMPLEX16 x 176 per block, nothing carried from block to block; the closed form is
 * given at sora_hip_tx11a44.  d_sees_next[b] != 0: block b's x[160] is block b + 1's first sample (the preamble's blocks 0..2, handed on as one burst); for the
 * last block of the call, or d_sees_next NULL, x[160] = 0. */
int sora_hip_upsample40to44(const sora_complex16* d_in, sora_complex16* d_out, const uint8_t* d_sees_next, size_t nblocks, void* stream);
/* TPackSample16to8 (brick/inc/stdbrick.hpp:415-445): COMPLEX16 -> COMPLEX8 with signed saturation (_mm_packs_epi16).  nsamples must be a multiple of 8, the brick's
 * burst (SORA_ERR_INVALID_PARAM otherwise). */
int sora_hip_pack16to8(const sora_complex16* d_in, int8_t* d_out, size_t nsamples, void* stream);
/* TTS11aSrc (preamble11a.hpp:19-140): the 640 COMPLEX16 preamble samples at 40 MHz, ncopies times back to back */
int sora_hip_preamble11a(sora_complex16* d_out, size_t ncopies, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The bricks of the 802.11n 2x2 modulation graphs as stage entry points: what CreatePreambleGraph11n, CreateSigGraph11n and CreateModGraph11n
 * (kernel/bb/demod11/fb11nmod_config.hpp) are built from beyond the 802.11a stages above, each with the port format of the brick it replaces:
 *     preamble11n(0)
 *     SIG:  conv_encode11a -> interleave11a -> sig_map11n -> add_pilot11a (bpsk_mod 30339) -> ifft_only11n -> chain 0 add_gi11n, chain 1 csd11n(2) + add_gi11n
 *     preamble11n(1)
 *     data: scramble11a -> conv_encode11a -> stream_parse11n -> per stream interleave11n -> map11n -> add_pilot11n -> ifft_only11n -> chain 1 csd11n(4) -> add_gi11n
 * T11aSc, TConvEncode_*, the SIG graph's T11aInterleaveBPSK and T11aAddPilot<30339> are the 802.11a stages; TBB11nSrc, TBB11nSigSrc and TBB11nMRSelect are the host's.
 * The conventions are those of the 802.11a block: device pointers, stream order, no allocation, no host wait; a null pointer or a symbol buffer that is not 16-byte
 * aligned gives SORA_ERR_INVALID_PARAM, no device SORA_ERR_NO_DEVICE, a count of 0 is SORA_OK and launches nothing.  Bits are packed in bytes, LSB first.
 * N_b = ceil(52 n_bpsc / 8) = 7, 13, 26, 39 bytes per stream and symbol; rows lie back to back, unpadded.  DESIGN.md section 7, f5b.
 * ------------------------------------------------------------------------------------------------ */
/* TStreamParser{BPSK,QPSK,QAM16,QAM64}_12 (Brick11/src/streamparser.hpp, _b_stream_parser.h): IPORT uchar x 13 n_bpsc -> OPORTS 0 and 1 uchar x N_b per symbol.
 * With s = max(1, n_bpsc / 2), coded bit k goes to stream (k / s) & 1 as its bit (k / 2s) s + k % s.  BPSK's seventh byte carries four bits: its upper half is 0
 * on both outputs, as the brick's half-byte table writes it. */
int sora_hip_stream_parse11n(const uint8_t* d_in, uint8_t* d_out0, uint8_t* d_out1, int n_bpsc, size_t nsym, void* stream);
/* T11nInterleave{BPSK,QPSK,QAM16,QAM64}_S1 / _S2 = T11Interleave<52 n_bpsc, n_bpsc, 13, 11, I_SS> (interleave.hpp:17-123): IPORT uchar x N_b -> OPORT uchar x N_b
 * per symbol.  spatial_stream as for sora_hip_deinterleave11n: 0 = _S1 (first stream), 1 = _S2.  The brick's table is indexed by whole input bytes; for BPSK its bits
 * 52..55 are ORed onto output positions below 52 (where its loop over k = 52..55 sends them) and output bits 52..55 are 0.  The parser leaves those input bits 0. */
int sora_hip_interleave11n(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, int spatial_stream, size_t nsym, void* stream);
/* TMap11a{BPSK,QPSK,QAM16,QAM64}<MOD> behind the 11n interleavers: IPORT uchar x N_b -> COMPLEX16 x 52 per symbol.  mod = the brick's MOD (1 .. 32767); 0 = what the
 * 802.11n graph instantiates: 30339, 21453, 9594, 4681.  For BPSK the brick emits 56 carriers per 7 bytes and T11nAddPilot discards the last four (ipin.clear(),
 * pilot_11n.hpp:78-79): this stage produces the 52 -- the one place where a stage's format is not the brick's pin. */
int sora_hip_map11n(const uint8_t* d_in, sora_complex16* d_out, int n_bpsc, int mod, size_t nsym, void* stream);
/* TSigMap11n (mapper11n.hpp): IPORT uchar x 18 -> OPORT COMPLEX16 x 144 per frame: bytes 0..5 (L-SIG) MapBPSK, +-30339 on I; bytes 6..17 (HT-SIG) MapQBPSK, on Q */
int sora_hip_sig_map11n(const uint8_t* d_in, sora_complex16* d_out, size_t nframes, void* stream);
/* T11nAddPilot<spatial_stream> (pilot_11n.hpp:7-82, _b_dot11_pilot.h): IPORT COMPLEX16 x 52 -> OPORT COMPLEX16 x 64 per symbol: data on bins 36..63 then 1..28
 * without +-7 and +-21, pilots 30339 x sign at 43, 57, 7, 21, every other bin 0.  The frame tables are sora_hip_add_pilot11a's; the symbol at position n of its frame
 * takes _pilot_sign[(n + 3) % 127] x _pilot[n & 3][spatial_stream][k].  Table entry f begins at position d_pos0[f] of its frame (d_pos0 NULL: 0 everywhere), as for
 * sora_hip_add_pilot11a_from.  Symbols that no frame owns are not written. */
int sora_hip_add_pilot11n(const sora_complex16* d_in, sora_complex16* d_out, const uint32_t* d_first, const uint32_t* d_nsym, const uint32_t* d_pos0,
                          size_t nframes, int spatial_stream, void* stream);
/* TIFFTxOnly (fft.hpp:63-103): IPORT COMPLEX16 x 64 -> OPORT COMPLEX16 x 128 per symbol: bins 0..31 and 32..63 at bins 0..31 and 96..127 of the reference's fixed-point
 * IFFT<128>; no shift, no guard interval, no window */
int sora_hip_ifft_only11n(const sora_complex16* d_in, sora_complex16* d_out, size_t nsym, void* stream);
/* TCSD<ncsd> (csd.hpp): COMPLEX16 x 128 -> 128 per symbol, output sample (i + 4 ncsd) mod 128 = input sample i.  ncsd 1 .. 31 (the graphs use 2 and 4).  Out of place
 * only: d_in == d_out gives SORA_ERR_INVALID_PARAM. */
int sora_hip_csd11n(const sora_complex16* d_in, sora_complex16* d_out, int ncsd, size_t nsym, void* stream);
/* TAddGI (gi.hpp): COMPLEX16 x 128 -> 160 per symbol: the last 32 samples, then the 128 */
int sora_hip_add_gi11n(const sora_complex16* d_in, sora_complex16* d_out, size_t nsym, void* stream);
/* LSrc (field 0: L-STF, L-LTF, 640 COMPLEX16 per chain) / HTSrc (field 1: HT-STF, HT-LTF1, HT-LTF2, 480 per chain) (preamble11n.hpp), ncopies times back to back into
 * d_out0 (TX chain 0) and d_out1 (chain 1): the fixed fields sora_hip_tx11n writes, from the same table */
int sora_hip_preamble11n(sora_complex16* d_out0, sora_complex16* d_out1, int field, size_t ncopies, void* stream);

/* 802.11n 2x2 transmitter: the reference's modulation graphs CreatePreambleGraph11n + CreateSigGraph11n + CreateModGraph11n
 * (kernel/bb/demod11/fb11nmod_config.hpp) as Test11N_FB_Mod runs them (fb11n_mod.cpp:28-70): L-STF, L-LTF, L-SIG, HT-SIG, HT-STF,
 * HT-LTF1, HT-LTF2, data; 20 MHz, long GI, MCS 8..14 (two spatial streams, one per TX chain), a batch of frames per call.
 * Frame f: MPDU WITHOUT FCS (the FCS is appended) of d_len[f] bytes at d_mpdu + d_off[f], MCS d_mcs[f], scrambler seed d_seed[f]
 * (d_seed NULL: 0xAB for every frame, what the reference harness uses, fb11nmod_config.hpp:51).  Writes sora_hip_tx11n_samples(len,
 * mcs) COMPLEX16 samples at 40 MHz per chain -- what the graph's sinks receive, GetSinkSampleCount(), without the 32 extra samples
 * fb11n_mod.cpp writes to its files -- at sample d_out_off[f] of d_out0 (TX chain 0) and of d_out1 (TX chain 1).
 * Accepted: MCS 8..14 and 1..4092 bytes without FCS; sora_hip_tx11n_samples is 0 for anything else (MCS 15 is routed to TDropAny by
 * the reference: no frame).  The MCS and length arrays are device memory: a frame whose MCS or length is not accepted gets nothing
 * written to its output range, and the other frames of the call are not affected.
 * The sample count follows the reference, not the standard: the data field has one symbol more than the standard's N_SYM whenever
 * N_SYM x N_DBPS is not a multiple of 8 (MCS 8, 10 and 14; ht_padding_bytes rounds the padded field up to whole bytes). */
size_t sora_hip_tx11n_samples(uint32_t mpdu_len_nofcs, uint32_t mcs);
int sora_hip_tx11n(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed,
                   size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, void* stream);

/* 40 MHz HT 2x2 transmitter: the frame the 40 MHz receiver below (sora_ht40_*) takes -- HT-mixed format, 40 MHz, two spatial streams,
 * long GI, MCS 8..14, a batch of frames per call.  PARITY UNPINNED, as for that receiver: the reference has no 40 MHz graph.  The format is
 * the one oracle/py_ht40.py (tx_frame) defines: L-STF 320, L-LTF 320, L-SIG 160, HT-SIG 2 x 160, HT-STF 160 samples (the 20 MHz legacy
 * waveforms on both halves of the channel, the upper half rotated by +90 degrees, identical on both chains, no cyclic shifts), then two
 * HT-LTF symbols (P = [[1, -1], [1, 1]]) and N_SYM = ceil((16 + 8 (len + 4) + 6) / N_DBPS) data symbols of 160 on 114 carriers; each spatial
 * stream carries its own PSDU through its own scrambler, encoder and interleaver and leaves on its own TX chain.  The waveform is that
 * model restated in integers (tests/tx_ht40_model.py) and held to it: every frequency-domain value times A = 16384 (an HT-LTF carrier),
 * rounded, every symbol through the reference's fixed-point IFFT<128>; this call equals the integer model sample for sample, and the
 * integer model equals tx_frame x A / 128 to within the transform's rounding (about 10 LSB at an rms of about 1200).
 * Frame f: two MPDUs WITHOUT FCS (the FCS is appended to each) of d_len[f] bytes each -- HT-SIG carries one LENGTH -- at d_mpdu +
 * d_off[2 f] (stream 0) and d_mpdu + d_off[2 f + 1] (stream 1), MCS d_mcs[f], scrambler seeds d_seed[2 f], d_seed[2 f + 1] (seven bits
 * used; d_seed NULL: 0x5D and 0x2B, the model's defaults).  Writes sora_hip_tx_ht40_samples(len, mcs) = 1280 + 160 (2 + N_SYM) COMPLEX16
 * samples at 40 MHz per chain at sample d_out_off[f] of d_out0 (TX chain 0) and of d_out1 (TX chain 1); HT-LTF 1 starts 1280 samples in
 * (sora_ht40_frame.offset).  Accepted: MCS 8..14 and 1..3996 bytes without FCS (LENGTH = len + 4 <= 4000, the receiver's limit; N_SYM =
 * sora_ht40_symbols(len + 4, len + 4, n_bpsc, code_rate)); sora_hip_tx_ht40_samples is 0 for anything else.  Null checks, error codes,
 * the behaviour without a device and "a frame that is not accepted gets nothing written, the others are not affected" are sora_hip_tx11n's. */
size_t sora_hip_tx_ht40_samples(uint32_t mpdu_len_nofcs, uint32_t mcs);
int sora_hip_tx_ht40(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed,
                     size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, void* stream);
/* The JOINT coding of the same frame (opt-in; DESIGN.md section 7 "g3"; the receiver takes it with sora_ht40_set_coding(rx, SORA_HT40_CODING_JOINT)).  As
 * oracle/py_ht40.py::tx_frame, except that a frame carries ONE PSDU of LENGTH = len + 4 <= 4000 bytes, the way IEEE 802.11n-2009 (N_ES = 1) and the reference's own
 * 20 MHz modulator (fb11nmod_config.hpp: one encoder, TStreamParser*) do it:
 *   - bit field: SERVICE(16) + PSDU + tail(6) + pad up to N_SYM x N_DBPS bits, N_DBPS = 2 x 108 x N_BPSC x R, N_SYM = ceil((16 + 8 LENGTH + 6) / N_DBPS)
 *     = sora_ht40_symbols_joint(LENGTH, n_bpsc, code_rate);
 *   - coding: one scrambler (one seed, seven bits used, default 0x5D; the tail forced to zero after scrambling), one K = 7 encoder, the same three puncturing patterns;
 *   - stream parser (the reference's rule, sora_hip_tx11n's): with s = max(1, N_BPSC / 2), coded bit kc (0 .. 2 N_CBPSS - 1) of a symbol goes to spatial stream
 *     (kc / s) & 1 and becomes that stream's bit (kc / 2s) s + kc % s;
 *   - unchanged: each stream's HT interleaver, mapper and carrier plan, the pilots, HT-LTFs, preamble, HT-SIG bits and the amplitudes A.  HT-SIG does not signal the
 *     coding: it is a property of the call here and of the handle at the receiver.  L-SIG's length follows from the new N_SYM by the same formula.
 * Frame f: one MPDU WITHOUT FCS of d_len[f] bytes at d_mpdu + d_off[f], MCS d_mcs[f], seed d_seed[f] (d_seed NULL: 0x5D).  Writes sora_hip_tx_ht40_joint_samples(len,
 * mcs) = 1280 + 160 (2 + N_SYM) samples per chain (0 outside MCS 8..14 and 1..3996 bytes).  Sample-exact against tests/ht40_joint_model.py::frame_int_joint.  Null
 * checks, error codes, the behaviour without a device and "a frame that is not accepted gets nothing written, the others are not affected" are sora_hip_tx_ht40's. */
size_t sora_hip_tx_ht40_joint_samples(uint32_t mpdu_len_nofcs, uint32_t mcs);
int sora_hip_tx_ht40_joint(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed,
                           size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, void* stream);
/* The SHORT GUARD INTERVAL of the same frames (opt-in; DESIGN.md section 7 "g4"; the library's own definition of IEEE 802.11n-2009's HT-mixed short GI at 40 MHz).  A
 * short-GI frame equals the long-GI frame of the same PSDUs, MCS and seeds up to and including HT-LTF 2 -- the legacy fields, HT-SIG, HT-STF and both HT-LTFs keep the
 * 32-sample cyclic prefix and 160-sample symbols -- except that
 *   - HT-SIG bit 31 (Short GI) is 1, and the CRC-8 over bits 0..33 follows;
 *   - L-SIG LENGTH follows tx_frame's rule with 4 x N_SYM replaced by 4 x ceil(9 N_SYM / 10): the data field's 3.6 us symbols rounded up to whole 4 us;
 * and every DATA symbol is 144 samples: the last 16 of the 128 transformed samples, then the 128 (no window, no cyclic shift, as before).  A frame is 1600 + 144 N_SYM
 * samples per chain; N_SYM, scrambling, coding, puncturing, stream parsing, interleaving, mapping and pilots are unchanged.
 * sora_hip_tx_ht40_gi has sora_hip_tx_ht40's arguments in its order plus d_gi, a guard-interval kind per frame (the shape of sora_hip_tx11b_pre's d_preamble): 0 = long
 * (sora_hip_tx_ht40's frame, sample for sample), 1 = short; d_gi NULL: every frame long.  Any other kind is treated like an MCS that is not accepted: _gi_samples
 * answers 0 and nothing is written for that frame.  sora_hip_tx_ht40_joint_gi is the same for the joint coding.  Sample-exact against tests/tx_ht40_gi_model.py.  The
 * receiver takes such frames as descriptors that carry SORA_HT40_SHORT_GI, or from raw captures with sora_ht40_set_guard(rx, SORA_HT40_GUARD_SIGNALLED). */
size_t sora_hip_tx_ht40_gi_samples(uint32_t mpdu_len_nofcs, uint32_t mcs, uint32_t gi);
int sora_hip_tx_ht40_gi(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed, const uint8_t* d_gi,
                        size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, void* stream);
size_t sora_hip_tx_ht40_joint_gi_samples(uint32_t mpdu_len_nofcs, uint32_t mcs, uint32_t gi);
int sora_hip_tx_ht40_joint_gi(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed, const uint8_t* d_gi,
                              size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, void* stream);
/* MCS 15 (two streams, 64-QAM, rate 5/6: SORA_CR_56 above): the _gi entry points' arguments plus a gate, int mcs_max.  14: the _gi entry
 * points' output byte for byte -- their kernels are launched, MCS 15 writes nothing and counts 0 samples.  15: MCS 15 is accepted as well, for 1..3996 bytes, in both
 * codings and both guard intervals: N_BPSC 6, N_DBPS = 540 per stream (1080 over the one field of the joint coding), N_SYM = ceil((16 + 8 (len + 4) + 6) / N_DBPS), the
 * encoder's output punctured to A1 B1 A2 B3 A4 B5 per five input bits (N_CBPS per stream, 648, is a whole number of such groups), HT-SIG's MCS field 15; everything
 * else in the header and in the frame is MCS 14's.  Any other gate is SORA_ERR_INVALID_PARAM (the _samples forms: 0).  sora_hip_tx_ht40, _joint and the _gi forms keep
 * refusing MCS 15.  What takes such frames: a receive handle after sora_ht40_set_mcs_max(rx, 15). */
size_t sora_hip_tx_ht40_mcs_samples(uint32_t mpdu_len_nofcs, uint32_t mcs, uint32_t gi, int mcs_max);
int sora_hip_tx_ht40_mcs(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed, const uint8_t* d_gi,
                         size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, int mcs_max, void* stream);
size_t sora_hip_tx_ht40_joint_mcs_samples(uint32_t mpdu_len_nofcs, uint32_t mcs, uint32_t gi, int mcs_max);
int sora_hip_tx_ht40_joint_mcs(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed, const uint8_t* d_gi,
                               size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, int mcs_max, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The bricks of the 40 MHz HT 2x2 modulation graph as stage entry points: what sora_hip_tx_ht40, _joint and _gi fuse, brick by brick, so that a host can replace ONE
 * brick, put its own between two of them, or pair the transmit bricks with the receive stages sora_hip_demap_ht40, _deinterleave_ht40 and _stream_join_ht40:
 *     preamble_ht40(0)
 *     SIG:  conv_encode11a (1/2) -> interleave11a (BPSK) -> sig_map_ht40 -> ifft_ht40 -> add_gi_ht40 (long); the same samples on both chains
 *     preamble_ht40(1)
 *     data, per-stream coding:  scramble11a -> conv_encode11a -> interleave_ht40_stream (iss) -> map_ht40 -> add_pilot_ht40 -> ifft_ht40 -> add_gi_ht40 (gi)
 *     data, joint coding:       scramble11a -> conv_encode11a -> stream_parse_ht40 -> interleave_ht40 (iss) -> map_ht40 -> add_pilot_ht40 -> ifft_ht40 -> add_gi_ht40 (gi)
 * The scrambler, the encoder and the SIG symbols' interleaver are the 802.11a stages above.  The scrambler's register for the transmitter's seed s (seven bits, bit i of
 * s = x[-1 - i], py_ht40.scramble_seq) is d_seed = bit-reversed-7(s) << 1; its TAIL_SCRAMBLE byte is the tail rule (the six tail bits start a byte).  The source of the
 * fields -- the 9 SIG bytes with the HT-SIG CRC-8, SERVICE + PSDU + FCS + tail + pad -- is the host's (sora_amd.mod_ht40_fields).
 * PARITY UNPINNED, as for the transmitter: the reference has no 40 MHz graph.  Each brick is defined by the project's integer model (tests/mod_ht40_model.py, from
 * tests/tx_ht40_model.py, ht40_joint_model.py and tx_ht40_gi_model.py) and is exact against it and against the fused kernels.
 * N_b40 = ceil(108 n_bpsc / 8) = 14, 27, 54, 81 bytes per stream and symbol; bits are packed LSB first, rows lie back to back, unpadded; the upper half of BPSK's 14th
 * byte is 0.  The conventions are those of the stage blocks above: device pointers, stream order, no allocation, no host wait; a null pointer or a symbol buffer that is
 * not 16-byte aligned gives SORA_ERR_INVALID_PARAM, a count of 0 is SORA_OK and launches nothing, no device SORA_ERR_NO_DEVICE; a bad n_bpsc, spatial_stream, gi or field
 * is refused before the count is looked at, as by the receive stages of this graph.  Symbols that no frame owns are not written.  DESIGN.md section 7, g2b.
 * ------------------------------------------------------------------------------------------------ */
/* The stream parser on the 216 n_bpsc coded bits of a symbol: IPORT uchar x 27 n_bpsc -> OPORTS 0 and 1 uchar x N_b40 per symbol.  With s = max(1, n_bpsc / 2), coded bit k
 * goes to stream (k / s) & 1 as its bit (k / 2s) s + k % s (sora_hip_stream_parse11n's rule, the inverse of sora_hip_stream_join_ht40). */
int sora_hip_stream_parse_ht40(const uint8_t* d_in, uint8_t* d_out0, uint8_t* d_out1, int n_bpsc, size_t nsym, void* stream);
/* The HT interleaver for 40 MHz (N_COL 18, N_ROW 6 n_bpsc, N_ROT 29): uchar x N_b40 -> uchar x N_b40 per symbol; the inverse of sora_hip_deinterleave_ht40's index map.
 * Input bit k < 108 n_bpsc of a row goes to bit r(k); BPSK's input bits 108..111 are not read. */
int sora_hip_interleave_ht40(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, int spatial_stream, size_t nsym, void* stream);
/* The same map reading by bit address, which is what lets sora_hip_conv_encode11a's output feed the per-stream chain: frame f's coded stream begins at byte d_in_off[f] of
 * d_in (no alignment asked); symbol j < d_nsym[f] of the frame reads bits 108 n_bpsc j onward of that stream (at BPSK odd symbols start mid-byte) and writes row
 * d_first[f] + j of d_out (16-byte aligned, rows of N_b40).  Rows that no frame owns are not written; a frame of 0 symbols writes nothing. */
int sora_hip_interleave_ht40_stream(const uint8_t* d_in, const uint32_t* d_in_off, const uint32_t* d_first, const uint32_t* d_nsym, uint8_t* d_out, int n_bpsc,
                                    int spatial_stream, size_t nframes, void* stream);
/* The mapper: uchar x N_b40 -> COMPLEX16 x 108 per symbol.  Carrier c takes bits c n_bpsc .. of the row, the first half for I and the second for Q, Gray, first bit = sign;
 * the odd integers times 6144, 6144, 4000, 2214 (n_bpsc 1, 2, 4, 6); BPSK on I alone. */
int sora_hip_map_ht40(const uint8_t* d_in, sora_complex16* d_out, int n_bpsc, size_t nsym, void* stream);
/* L-SIG and HT-SIG: uchar x 18 per frame (three interleaved BPSK symbols of 48 bits) -> COMPLEX16 x 3 x 128 bins per frame, complete: the 48 carriers +-16384 (L-SIG on I,
 * HT-SIG 1 and 2 on Q) and the pilots +, +, +, - x 16384 on I at legacy carriers -21, -7, 7, 21, all on both halves of the channel (carrier k at bin k - 32 and, times j,
 * at bin k + 32); every other bin 0. */
int sora_hip_sig_map_ht40(const uint8_t* d_in, sora_complex16* d_out, size_t nframes, void* stream);
/* COMPLEX16 x 108 -> COMPLEX16 x 128 bins per symbol: data carrier c at its bin (carriers -58..-2, 2..58 without the pilots'), pilots (12288, 0) at carriers +-11, +-25, +-53,
 * the 14 other bins 0.  Frame f owns symbols d_first[f] .. d_first[f] + d_nsym[f] - 1 (sora_hip_add_pilot11a's tables). */
int sora_hip_add_pilot_ht40(const sora_complex16* d_in, sora_complex16* d_out, const uint32_t* d_first, const uint32_t* d_nsym, size_t nframes, void* stream);
/* The reference's fixed-point IFFT<128> of 128 bins in natural order: COMPLEX16 x 128 -> COMPLEX16 x 128 per symbol, no shift, no guard interval, no window */
int sora_hip_ifft_ht40(const sora_complex16* d_in, sora_complex16* d_out, size_t nsym, void* stream);
/* The guard interval: COMPLEX16 x 128 -> x 160 (gi 0: the last 32 samples, then the 128) or x 144 (gi 1: the last 16, then the 128) per symbol.  Any other gi gives
 * SORA_ERR_INVALID_PARAM. */
int sora_hip_add_gi_ht40(const sora_complex16* d_in, sora_complex16* d_out, int gi, size_t nsym, void* stream);
/* The fixed fields sora_hip_tx_ht40 writes, from the same per-device table: field 0 = L-STF, L-LTF (640 COMPLEX16 per chain), field 1 = HT-STF, HT-LTF1, HT-LTF2 (480 per
 * chain), ncopies times back to back into d_out0 (TX chain 0) and d_out1 (chain 1).  The first call on a device builds the table and waits for it. */
int sora_hip_preamble_ht40(sora_complex16* d_out0, sora_complex16* d_out1, int field, size_t ncopies, void* stream);

/* 802.11b transmitter: the reference's modulation graph CreateModGraph (kernel/bb/demod11/fb11bmod_config.hpp:28-50) as
 * Test11B_FB_Mod runs it (fb11b_mod.cpp:40-70): long preamble (SYNC, SFD), PLCP header, MPDU + FCS at 1, 2, 5.5 or 11 Mbps, Barker
 * DBPSK / DQPSK or CCK, TQuickPulseShaper; a batch of frames per call.
 * Frame f: MPDU WITHOUT FCS (the FCS is appended) of d_len[f] bytes at d_mpdu + d_off[f], rate d_rate_kbps[f] (1000, 2000, 5500 or
 * 11000).  Writes sora_hip_tx11b_samples(len, rate) COMPLEX8 samples at 44 MHz -- what TModSink receives, tx_sample_cnt() -- at sample
 * d_out_off[f] of d_out (64-bit offsets: a batch may exceed 2^31 samples).
 * Accepted: those four rates and 1..4092 bytes without FCS; sora_hip_tx11b_samples is 0 for anything else.  The rate and length
 * arrays are device memory: a frame whose rate or length is not accepted gets
 * nothing written (its output range and d_phase_out[f] stay as they are), and the other frames of the call are not affected.
 * Differential phase: the reference's four spreaders share CF_DifferentialMap::last_phase (0: 0, 1: -pi/2, 2: pi/2, 3: pi), and no
 * reset touches it, so one reference process carries it from frame to frame; the preamble reads only its low bit, so a frame comes out
 * as W or -W.  d_phase_in[f] is last_phase when frame f starts (d_phase_in NULL: 0, a fresh reference process); d_phase_out, if not
 * NULL, receives last_phase after frame f.  Frames of one call are independent: a host chains calls by passing d_phase_out back as
 * d_phase_in.  Sample count: 192 x 44 + (len + 4) x S + 24, S = 352, 176, 64, 32 samples a byte at 1, 2, 5.5, 11 Mbps; the 24
 * are the shaper's five flush steps and TPackSample16to8's padding of its last burst. */
size_t sora_hip_tx11b_samples(uint32_t mpdu_len_nofcs, uint32_t rate_kbps);
int sora_hip_tx11b(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps,
                   const uint8_t* d_phase_in, uint8_t* d_phase_out, size_t nframes,
                   int8_t* d_out, const uint64_t* d_out_off, void* stream);
/* The same with a preamble kind per frame: d_preamble[f] = 0, the long preamble (sora_hip_tx11b's frame, byte for byte), or 1, the SHORT
 * preamble, which the reference's source brick refuses (TBB11bSrc::PreparePLCPHeader, PHY_11b.hpp:115-119: "not supported yet") although
 * TBB11bMRSelect already counts its header bytes (:224-229) and kernel/inc/dot11_plcp.h holds its constants.  Short PPDU: SYNC = 7 bytes of
 * 0x00, SFD 0x05CF (bytes 0xCF, 0x05), both at 1 Mbps DBPSK; the six PLCP header bytes (built as for the long preamble) at 2 Mbps DQPSK;
 * MPDU + FCS at 2000, 5500 or 11000 kbps (1000 is not accepted behind a short preamble); the scrambler starts from 0x1B; the differential
 * phase runs on from SFD to header to payload, d_phase_in / d_phase_out as above.  Sample count: 96 x 44 + (len + 4) x S + 24.
 * d_preamble NULL: every frame long, sora_hip_tx11b itself.  A kind other than 0 or 1 is treated like a rate that is not accepted:
 * sora_hip_tx11b_pre_samples is 0 and nothing is written. */
size_t sora_hip_tx11b_pre_samples(uint32_t mpdu_len_nofcs, uint32_t rate_kbps, uint32_t preamble);
int sora_hip_tx11b_pre(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps, const uint8_t* d_preamble,
                       const uint8_t* d_phase_in, uint8_t* d_phase_out, size_t nframes,
                       int8_t* d_out, const uint64_t* d_out_off, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The bricks of the 802.11b modulation graph as stage entry points: what CreateModGraph (kernel/bb/demod11/fb11bmod_config.hpp:28-50) is built from, each with the
 * ports of the brick it replaces, so that a host can replace ONE brick, or compose the graph from stages (sora_amd.mod11b_by_stages does):
 *     ppdu -> sc741 -> dbpsk_spread / dqpsk_spread / cck5_encode / cck11_encode -> pulse_shape -> pack16to8 (sora_hip_pack16to8, above)
 * TBB11bMRSelect only routes and stays the host's; TModSink is the caller's buffer.  The conventions are those of the 802.11b receive stages below: device pointers,
 * stream order, no allocation, no host wait; a null pointer gives SORA_ERR_INVALID_PARAM (sora_hip_last_error() names the function), no device SORA_ERR_NO_DEVICE,
 * nstreams = 0 is SORA_OK and launches nothing.  The bricks are stateful streams, so a call works on a BATCH of independent streams described by device tables: stream f
 * owns d_n[f] input units (bytes; chips for the shaper) starting at ELEMENT d_first[f] of d_in and writes its output from element d_out_first[f] of d_out (bytes,
 * COMPLEX8 chips, COMPLEX16 samples).  What the brick keeps lies in a per-stream record of 32-bit words that the call reads and writes back: the state after the call
 * is the state the brick would hold, the same stream cut into two calls gives what one call gives, output and state, and bytes of d_out that no stream owns are not
 * written.  A stream with d_n[f] = 0 leaves its record as it is.  max_n bounds every d_n[f] (units of a stream at or behind it are not touched; at most 2^24).  Offsets
 * need no alignment beyond their element's (d_in / d_out themselves: their element's).  A workgroup walks one stream, kMod11bT = 1024 units a pass, 16 bytes per lane
 * and store.  Every stage equals tests/mod11b_model.py bit for bit, output and record (tests/test_gpu_mod11b_stages.py).  Measured on one MI355X on the commit that
 * adds them (parent b2fead2), 4096 streams of a 1500-byte frame per call (tools/bench_mod11b_stages.py, profiles/mod11b_stages.json): the spreaders 0.224 / 0.122 /
 * 0.045 / 0.033 ms at 1 / 2 / 5.5 / 11 Mbps (62 / 57 / 58 / 40 % of the HBM peak), the shaper 2.76 / 1.36 / 0.47 / 0.24 ms (45-47 %) beside sora_hip_pack16to8's 75 %
 * in the same run, ppdu and sc741 0.024 ms each; composed they take 4.8 to 5.9 times sora_hip_tx11b's time.  DESIGN.md section 7, f6b.
 * ------------------------------------------------------------------------------------------------ */
/* CF_DifferentialMap::last_phase (0: 0, 1: -pi/2, 2: pi/2, 3: pi; context: no Reset clears it), which the four spreaders share, and TCCK11Encode's bEven (brick
 * state, 0 after Reset).  Each stage reads and writes its own fields and leaves the others alone. */
typedef struct { uint32_t last_phase, is_even, reserved[2]; } sora_mod11b_state;
/* TQuickPulseShaper's m_temps[0..3]: the partial sums of the next four bursts (its fifth row is never written and stays 0).  All 0 after Reset. */
typedef struct { sora_complex16 temps[4][4]; } sora_shaper11b_state;
/* TBB11bSrc (PHY_11b.hpp:19-206) with the preamble kind per frame of sora_hip_tx11b_pre: frame f's MPDU WITHOUT FCS, d_len[f] bytes at d_mpdu + d_off[f] -> the PPDU
 * bytes the source brick emits, from byte d_out_first[f] of d_out: SYNC, SFD, SIGNAL, SERVICE, LENGTH, CRC-16, MPDU, FCS -- 24 + len + 4 bytes behind the long preamble
 * (d_preamble[f] = 0), 15 + len + 4 behind the short one (1).  A frame that sora_hip_tx11b_pre_samples answers with 0 gets nothing written. */
int sora_hip_ppdu11b(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps, const uint8_t* d_preamble, uint8_t* d_out,
                     const uint32_t* d_out_first, size_t nframes, void* stream);
/* TSc741 (scramble.hpp:7-88), 1 -> 1 byte.  d_reg[f]: the 7-bit register; after Reset it is the context's sc_seed, 0x6C behind the long preamble and 0x1B behind the
 * short one.  Only the low 7 bits are read: the reference indexes a [256][128] table, so a larger value is out of ITS bounds. */
int sora_hip_sc741_11b(const uint8_t* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, uint32_t* d_reg, uint8_t* d_out,
                       size_t nstreams, size_t max_n, void* stream);
/* TBB11bDBPSKSpread (barkerspread.hpp:9-111), 1 byte -> 88 COMPLEX8 (d_out: re, im pairs; d_out_first in COMPLEX8): reads only last_phase & 1 and leaves 0 or 3.
 * TBB11bDQPSKSpread (:113-225), 1 -> 44: reads last_phase & 3. */
int sora_hip_dbpsk_spread11b(const uint8_t* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_mod11b_state* d_state, int8_t* d_out,
                             size_t nstreams, size_t max_n, void* stream);
int sora_hip_dqpsk_spread11b(const uint8_t* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_mod11b_state* d_state, int8_t* d_out,
                             size_t nstreams, size_t max_n, void* stream);
/* TCCK5Encode (cck.hpp:880-953), 1 byte -> 16 COMPLEX8; TCCK11Encode (:782-870), 1 -> 8, whose bEven (is_even, low bit read) flips with every byte.  last_phase: the
 * low two bits are read (the bricks index their tables with it unmasked). */
int sora_hip_cck5_encode11b(const uint8_t* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_mod11b_state* d_state, int8_t* d_out,
                            size_t nstreams, size_t max_n, void* stream);
int sora_hip_cck11_encode11b(const uint8_t* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_mod11b_state* d_state, int8_t* d_out,
                             size_t nstreams, size_t max_n, void* stream);
/* TQuickPulseShaper (pulse.hpp:254-384), 1 COMPLEX8 -> 4 COMPLEX16: ANY COMPLEX8, -128 included, with QuickShape's arithmetic (mul_low, wrapping 16-bit adds).  The
 * record holds the brick's PARTIAL SUMS, not past inputs, and one that no input history produces is honoured: sample s of step m of the call is
 * wrap16(temps[m][s] (m < 4) + sum_{j = 0 .. min(m, 4)} x[m - j] tap[4 j + s]).  d_flush (may be NULL: no stream flushes): d_flush[f] != 0 runs the brick's Flush behind
 * the stream's chips, five more bursts from zero input -- the stream then writes 4 (d_n[f] + 5) samples (and d_n[f] = 0 is five bursts from the record). */
int sora_hip_pulse_shape11b(const int8_t* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, const uint8_t* d_flush,
                            sora_shaper11b_state* d_state, sora_complex16* d_out, size_t nstreams, size_t max_n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 802.11n 2x2, stage level (the whole-path graph is sora_rx11n_* below).  Batched bricks, n symbols per call:
 * T11nDemap{BPSK,QPSK,QAM16,QAM64} (kernel/bb/Brick11/src/demapper11n.hpp:89-309): IPORT COMPLEX16 x 64 (one pilot-tracked
 * symbol of one spatial stream) -> OPORT uint8 x 52*N_BPSC soft values 0..7;
 * T11nDeinterleave{...}_S0/_S1 (deinterleaver_11n.hpp:4-1618): 52*N_BPSC soft values of spatial stream 0 or 1 -> de-interleaved.
 * All of CreateDemodGraph11n (fb11ndemod_config.hpp:166-264) stands here as stages, so that a host can replace ONE brick, or compose the graph (sora_amd.rx11n_by_stages):
 *     ingest (TDownSample2) -> cca | cfo_est -> freq_comp -> fft64 -> siso_est                                                   (carrier sense, L-LTF)
 *                                  | freq_comp -> data_symbol -> fft64 -> siso_comp (MRC) -> sig_demap -> sig_decode              (L-SIG, HT-SIG)
 *                                                                      -> mimo_est                                               (HT-LTF)
 *                                                                      -> mimo_comp -> pilot_track -> demap -> deinterleave -> stream_join -> viterbi11n_ws -> desc11a -> frame_sink11a
 * RxSwitch, T11nSymSel, T11nRxRateSel, Mimo64Join and TStreamFork only route and stay the host's.
 * ------------------------------------------------------------------------------------------------ */
int sora_hip_demap11n(const sora_complex16* d_in, uint8_t* d_soft, int n_bpsc, size_t n, void* stream);
int sora_hip_deinterleave11n(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, int spatial_stream, size_t n, void* stream);
/* TMimoChannelEst (channel_11n.hpp:329-443), a batch of frames: d_ltf_r[f][128] = the two HT-LTF symbols of RX chain r after the
 * FFT (first 64, second 64) -> CF_ChannelMimo per frame: d_h[f][2][128] (row = RX chain; columns 0..63 / 64..127 = spatial stream
 * 1 / 2) and d_hinv[f][2][128] = its 2x2 inverse x 2^16 per carrier, computed in single-precision floats operation for operation as
 * the reference's SSE code (brick/inc/sora_matrix.h:134-148,305-313) and packed with saturation.
 * TMimoChannelComp (channel_11n.hpp:445-521), a batch of symbols: x = (Hinv y) >> 9 with saturation; symbol s uses
 * d_hinv[d_frame_index[s]] (d_frame_index NULL: frame 0); y_r = RX chain r after the FFT, x_k = spatial stream k. */
/* The CFO / phase bricks (Brick11/src/dsp_math.h tables, generated with the C library as the reference does at start-up).
 * d_state[f][24] = CF_FreqOffset_11n of frame f: vfo_delta_i[8] | vfo_step_i[8] | vfo_theta_i[8] (int16).
 * sora_hip_cfo_est11n     TFreqEstimator_11n (freqoffset_11n.hpp:42-160): d_lltf_r[f][128] = the L-LTF of RX chain r (two 64-sample
 *                         halves) -> d_state[f] (vfo_delta_i = {0..7} x CFO, vfo_step_i = 8 x CFO, vfo_theta_i = 0; CFO_est = state[1])
 * sora_hip_freq_comp11n   TFreqComp_11n (freqoffset_11n.hpp:162-280): frame f owns d_nbursts[f] bursts of 8 samples starting at sample
 *                         d_first[f] of both chains; out = sat((in * sincos(vfo_delta_i - vfo_theta_i)) >> 15); vfo_delta_i advances by
 *                         vfo_step_i per burst and is written back.  max_bursts >= every d_nbursts[f].
 * sora_hip_pilot_track11n TPilotTrack_11n (pilot_11n.hpp:84-141): frame f owns symbols d_first[f] .. +d_nsym[f]-1 of the two spatial
 *                         streams (after TMimoChannelComp); vfo_theta_i of d_state[f] accumulates the mean pilot phase; d_theta[s][8]
 *                         (optional) receives vfo_theta_i as it stands after symbol s. */
int sora_hip_cfo_est11n(const sora_complex16* d_lltf0, const sora_complex16* d_lltf1, int16_t* d_state, size_t nframes, void* stream);
int sora_hip_freq_comp11n(const sora_complex16* d_in0, const sora_complex16* d_in1, sora_complex16* d_out0, sora_complex16* d_out1,
                          const uint32_t* d_first, const uint32_t* d_nbursts, int16_t* d_state, size_t nframes, size_t max_bursts, void* stream);
int sora_hip_pilot_track11n(const sora_complex16* d_x0, const sora_complex16* d_x1, const uint32_t* d_first, const uint32_t* d_nsym, int16_t* d_state,
                            int16_t* d_theta, size_t nframes, void* stream);
/* The legacy part of the HT-mixed preamble (both RX chains), a batch of frames:
 * sora_hip_siso_est11n   TSisoChannelEst (channel_11n.hpp:33-231): d_lltf_r[f][128] = the two L-LTF symbols of chain r after the FFT ->
 *                        d_ch[f][2][64], 1 / H per chain in Q16 with the reference's rounding lanes; bins 28..35, which the brick
 *                        leaves unwritten, are 0.
 * sora_hip_siso_comp11n  TSisoChannelComp (channel_11n.hpp:233-297) + TMrcCombine (PHY_11n.hpp:362-398): x_r = sat((y_r c_r) >> 9),
 *                        mrc = (x_0 + x_1) >> 1; symbol s uses d_ch[d_frame_index[s]] (NULL: frame 0); any of d_x0 / d_x1 / d_mrc may be
 *                        NULL (not all three).
 * sora_hip_sig_demap11n  T11nSigDemap (demapper11n.hpp:6-87): d_sym[f][3][64] = L-SIG, HT-SIG1, HT-SIG2 after MRC -> d_soft[f][144]
 *                        (L-SIG demapped on I, the HT-SIG symbols on Q; 48 carriers each). */
int sora_hip_siso_est11n(const sora_complex16* d_lltf0, const sora_complex16* d_lltf1, sora_complex16* d_ch, size_t nframes, void* stream);
int sora_hip_siso_comp11n(const sora_complex16* d_ch, const uint32_t* d_frame_index, const sora_complex16* d_y0, const sora_complex16* d_y1,
                          sora_complex16* d_x0, sora_complex16* d_x1, sora_complex16* d_mrc, size_t nsym, void* stream);
int sora_hip_sig_demap11n(const sora_complex16* d_sym, uint8_t* d_soft, size_t nframes, void* stream);
/* sora_hip_sig_decode11n  T11aDeinterleaveBPSK x3 -> T11nViterbiSig (viterbi.hpp:51-99) -> T11nSigParser (PHY_11n.hpp:432-513):
 *                        d_soft[f][144] (sora_hip_sig_demap11n's output) -> d_rec[f][12] = error_code (0 or SORA_E_PLCP_HEADER_FAIL),
 *                        data_rate_kbps, frame_length, ht_frame_mcs, ht_frame_length, code_rate, total_symbols, remain_symbols,
 *                        symbol_type (the context fields, from 0, as the parser leaves them -- partial on a failed parse),
 *                        then the decoded L-SIG (24 bits) and HT-SIG (bits 0..31, bits 32..41). */
int sora_hip_sig_decode11n(const uint8_t* d_soft, uint32_t* d_rec, size_t nframes, void* stream);
int sora_hip_mimo_est11n(const sora_complex16* d_ltf0, const sora_complex16* d_ltf1, sora_complex16* d_h, sora_complex16* d_hinv, size_t nframes, void* stream);
int sora_hip_mimo_comp11n(const sora_complex16* d_hinv, const uint32_t* d_frame_index, const sora_complex16* d_y0, const sora_complex16* d_y1,
                          sora_complex16* d_x0, sora_complex16* d_x1, size_t nsym, void* stream);

/* ---- The bricks that complete the graph.  Conventions: those of the 802.11b receive stage block below (above sora_hip_dc_remove11b): device pointers, stream order, no
 * allocation, no host wait; a null pointer gives SORA_ERR_INVALID_PARAM before any device work (sora_hip_last_error() names the function), no device SORA_ERR_NO_DEVICE, a count of
 * 0 is SORA_OK and launches nothing; a stateful brick works on a batch of independent streams described by device tables, with a per-stream record of 32-bit words that is read
 * and written back, and the same stream cut into two calls gives what one call gives.  Every stage equals tests/rx11n_stage_model.py bit for bit
 * (tests/test_gpu_11n_rx_stages.py).  DESIGN.md section 7, f1b. */
#define SORA_CCA11N_REARM 1u
/* TCCA11n (Brick11/src/cca_11n.hpp) with its MimoAutoCorr (autocorr.hpp:5-147).  The record holds the context fields the brick touches (cca_state: 0 power_clear, 1
 * power_detected; error_code; cca_pwr_reading), its three counters, his_index, the ring his_moving_energy as 64 pairs of words (low, high), a `timeouts` count
 * (SORA_CCA11N_REARM), and, in place of MimoAutoCorr's sample, product and sum arrays, the last 64 samples of both chains that the brick has consumed, oldest first: from a
 * constructed brick the wrapping moving sums are the sums of the last 32 products mod 2^32, so the samples determine them.  The record's domain is therefore the states
 * reachable from a constructed brick.
 *   as constructed:  every word 0, but the 64 ring entries, which are LLONG_MAX (0xFFFFFFFF, 0x7FFFFFFF) -- "prevent initial fake trigger" -- (sora_amd.cca11n_states makes them)
 *   after Reset():   sense_count, peak_found, peak_count = 0; everything else stands (cca_state and error_code are the context's: BB11nDemodCtx.Reset clears them) */
typedef struct {
    uint32_t cca_state, error_code, cca_pwr_reading, sense_count, peak_found, peak_count, his_index, timeouts;
    uint32_t his_moving_energy[64][2];
    sora_complex16 history[2][64];
} sora_cca11n_state;
/* d_in0 / d_in1: the two RX chains at 20 MHz (behind TDownSample2).  A unit is the brick's burst: 4 samples of both chains.  Stream f consumes bursts from SAMPLE d_first[f]
 * of both buffers, d_n[f] at most, until cca_state is power_detected or an error stands; d_used[f] = the bursts consumed, the deciding one included (the brick leaves the
 * rest of that burst unlooked at and unrecorded in the ring; the auto-correlator has seen it).  A stream that enters with power detected or an error standing consumes nothing.
 * flags 0: SORA_E_CS_TIMEOUT (defined with the 802.11b stages below; here: sense_count >= 84 at the end of a burst) stands and the stream ends there, as in
 * sora_hip_energy_detect11b.  SORA_CCA11N_REARM: the time-out does not stand -- the brick's _reset() is
 * applied, as RxThread does after the event (fb11n_demod.cpp:60-66), `timeouts` counts it, and the stream goes on.  max_n bounds every d_n[f] (< 2^30). */
int sora_hip_cca11n(const sora_complex16* d_in0, const sora_complex16* d_in1, const uint32_t* d_first, const uint32_t* d_n, sora_cca11n_state* d_state, uint32_t* d_used,
                    size_t nstreams, size_t max_n, unsigned flags, void* stream);
/* T11nDataSymbol (PHY_11n.hpp:288-356), 2 x 80 -> 2 x 64: frame f owns d_nsym[f] symbols of 80 samples from SAMPLE d_first[f] of both chains (no alignment beyond a
 * sample's); samples 16..79 of symbol k go to SYMBOL d_out_first[f] + k of d_out0 / d_out1, 64 samples each: the layout sora_hip_fft64 reads.  The brick's remain_symbols
 * count-down and its Flush at zero are the host's.  max_nsym >= every d_nsym[f]; at most 65535 frames per call. */
int sora_hip_data_symbol11n(const sora_complex16* d_in0, const sora_complex16* d_in1, const uint32_t* d_first, const uint32_t* d_nsym, const uint32_t* d_out_first,
                            sora_complex16* d_out0, sora_complex16* d_out1, size_t nframes, size_t max_nsym, void* stream);
/* TStreamJoin<2, 52 N_BPSC> -> TStreamConcat<2, s> (brick/inc/stdbrick.hpp:640-720), s = max(N_BPSC / 2, 1) as the graph wires it (StreamConcat_1 for BPSK and QPSK, _2
 * for 16-QAM, _3 for 64-QAM): d_s0 / d_s1 [n][52 N_BPSC] = the de-interleaved soft values of spatial stream 0 / 1 (sora_hip_deinterleave11n) -> d_out[n][104 N_BPSC] in groups of
 * s bytes, alternating stream 0, stream 1: byte for byte one job's soft values for sora_hip_viterbi11n_ws.  n_bpsc 1, 2, 4 or 6, else SORA_ERR_INVALID_PARAM. */
int sora_hip_stream_join11n(const uint8_t* d_s0, const uint8_t* d_s1, uint8_t* d_out, int n_bpsc, size_t n, void* stream);
/* T11aDesc (scramble.hpp:269-355), the descrambler of the 802.11a and the 802.11n graph: frame i reads d_len[i] + 2 decoded bytes at d_dec + d_off[i] -- what the trellis stages
 * write --, drops byte 0, seeds the register with byte 1 >> 1 and writes d_len[i] descrambled bytes at d_out + d_out_off[i]. */
int sora_hip_desc11a(const uint8_t* d_dec, const uint32_t* d_off, const uint32_t* d_len, uint8_t* d_out, const uint32_t* d_out_off, size_t n, void* stream);
/* TBB11aFrameSink (PHY_11a.hpp:609-700) over one frame each: d_len[i] = frame_length (a ushort: the low 16 bits) descrambled bytes at d_bytes + d_off[i] -> d_rec[i]:
 * error_code SORA_E_FRAME_OK / SORA_E_CRC32_FAIL and frame_crc32 = the frame's last four bytes as the brick reads them (little-endian).  Lengths below 4: the brick compares
 * byte_count with (ulong)(frame_length - 4), which has wrapped, so every byte goes into the CRC and it never decides: the record is 0, 0. */
typedef struct { uint32_t error_code, frame_crc32; } sora_sink11a_rec;
int sora_hip_frame_sink11a(const uint8_t* d_bytes, const uint32_t* d_off, const uint32_t* d_len, sora_sink11a_rec* d_rec, size_t n, void* stream);

/* ---- The front end of the 802.11a receive graph (CreateDemodGraph11a_40M, fb11ademod_config.hpp:169-232) as stages: what stands in front of sora_hip_lts11a and the
 * symbol chain, and the SIGNAL symbol's decoder and parser.  With them the graph reads
 *     dc_remove11a -> cca11a -> dc_estimate11a  (or carrier_sense11a: the three with the loop closed) | lts11a | data_symbol11a -> freq_comp11a -> fft64 -> equalize11a ->
 *     phase_comp11a -> pilot11a -> demap11a -> deinterleave11a -> viterbi_sig11a -> plcp_parse11a | .. -> viterbi11a -> desc11a -> frame_sink11a
 * TBB11bRxSwitch, T11aSymSelEx, TBB11aRxRateSel, TNoInline, TThreadSeparator and TDropAny only route and stay the host's.  The conventions are those stated above
 * sora_hip_cca11n and sora_hip_dc_remove11b: device pointers, stream order, no allocation, no host wait; a null pointer gives SORA_ERR_INVALID_PARAM before any device work
 * (sora_hip_last_error() names the function), no device SORA_ERR_NO_DEVICE, a count of 0 is SORA_OK and launches nothing; a stateful brick works on a batch of independent
 * streams described by the device tables d_first (SAMPLE index, no alignment) / d_n (bursts of 4 samples), max_n bounding every d_n[f] (bursts at or behind it are not
 * touched; max_n = 0 launches nothing and writes nothing, d_used and d_npass included), with a per-stream record of 32-bit words that is read and written back,
 * and the same stream cut into two calls gives what one call gives.  Every stage equals tests/rx11a_stage_model.py bit for bit (tests/test_gpu_11a_rx_stages.py).  DESIGN.md section 7, f2b. */
#define SORA_CCA11A_STOP_ON_TIMEOUT 1u
/* TDCRemoveEx<4>::Filter (brick/inc/dc.hpp:46-86), 4 -> 4: out = rep_sub(in, DC), 16-bit wrapping, with DC = d_dc[f] in all four elements (what CF_VecDC holds from its Reset
 * on: TDCEstimator adds the same value to all four).  That is TDCRemove's arithmetic bit for bit, sora_hip_dc_remove11b's; as there, d_out_first[f] is a SAMPLE
 * index.  The kernel is this entry's own because it stops a stream at max_n, which the 802.11b stage (whole 256-sample chunks) does not.  At most 65535 streams per call. */
int sora_hip_dc_remove11a(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, const sora_complex16* d_dc,
                          sora_complex16* d_out, size_t nstreams, size_t max_n, void* stream);
/* TDCEstimator (dc.hpp:99-165), 4 -> pass-through (not copied): sum_dc += hadd(in >> 5) per burst; the burst that finds update_cnt == 0 adds sum_dc >> 2 to DC, clears
 * sum_dc and sets update_cnt to 8; every burst then decrements it.  All 16-bit wrapping.  sum_dc and dc are one element of the brick's vectors (the four are equal).
 *   as constructed / after Reset():  update_cnt = 8, sum_dc = 0; dc stands (CF_VecDC::Reset makes it 0).  Domain: update_cnt 0 .. 8. */
typedef struct { uint32_t update_cnt; sora_complex16 sum_dc, dc; uint32_t reserved; } sora_dcest11a_state;
int sora_hip_dc_estimate11a(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, sora_dcest11a_state* d_state, size_t nstreams, size_t max_n, void* stream);
/* TCCA11a (Brick11/src/cca.hpp:104-441) alone, over DC-removed bursts at 20 MHz.  The record: the context fields the brick touches -- cca_state (0 power_clear, 1
 * power_detected), error_code, cca_pwr_threshold (read only), cca_pwr_reading, cca_peak_index --, its members sync_state (0 no_energy, 1 high_energy), auto_count,
 * sense_count, high_count, peak_corr, peak_index, sample_his as 16 samples in time order, already >> 2, and the three four-deep windows, oldest first, with their
 * accumulators.  The brick's unused members (ac_norm_his, energy_sqr_his, dc_est) are not part of it.
 *   as constructed:  every word 0 (a fresh context: cca_pwr_threshold is the host's; the reference harness sets 1000 * 1000)
 *   after Reset():   __init (cca.hpp:279-295): sync_state, auto_count, sense_count, high_count, peak_corr, peak_index, sample_his and the three windows with their sums 0;
 *                    the five context words stand (BB11aDemodContext::Reset clears cca_state and error_code)         (sora_amd.cca11a_states / cca11a_reset make both)
 *   domain:          every record a brick can hold: sync_state 0 / 1, peak_index 0 .. 15, each sum the wrapping sum of its window; otherwise any words -- auto_count > 0,
 *                    a lock held, a dropped lock's stale peak_corr / peak_index / high_count, a time-out standing.
 * Stream f consumes bursts until cca_state becomes power_detected or d_n[f] runs out; d_used[f] = the bursts consumed, the deciding one included.  A stream that enters with
 * power detected consumes nothing.  The gated output -- the bursts behind which sync_state is no_energy, which is what the brick hands to TDCEstimator -- is written
 * compacted from BURST d_out_first[f] of d_out (room for d_n[f] bursts), their count in d_npass[f].
 * Time-out, as the brick has it: sense_count >= 84 with no_energy at the end of a burst sets error_code = SORA_E_CS_TIMEOUT, and the walk goes on (the brick never looks at
 * error_code).  SORA_CCA11A_STOP_ON_TIMEOUT: the stream ends behind the burst that CHANGES error_code to it; a stream that enters with the time-out standing is not stopped
 * by it again.  Clearing it and applying Reset is the host's, as RxThread does at the end of the source call (fb11a_demod.cpp:47-57). */
typedef struct {
    uint32_t cca_state, error_code, cca_pwr_threshold, cca_pwr_reading, cca_peak_index;
    uint32_t sync_state, auto_count, sense_count, high_count; int32_t peak_corr; uint32_t peak_index, reserved0;
    sora_complex16 sample_his[16];
    int32_t ac_re[4], ac_im[4], energy[4], ac_re_sum, ac_im_sum, energy_sum; uint32_t reserved1;
} sora_cca11a_state;
int sora_hip_cca11a(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_cca11a_state* d_state, sora_complex16* d_out,
                    uint32_t* d_used, uint32_t* d_npass, size_t nstreams, size_t max_n, unsigned flags, void* stream);
/* The loop TDCRemoveEx -> TCCA11a -> TDCEstimator as ONE entry over RAW bursts: the estimate feeds back into the subtraction every eight gated bursts, so separate calls
 * have to be cut at each update.  d_used, the time-out and the flag as sora_hip_cca11a; no sample output.  Words 0-39 of the receive handle's continuation record
 * (sora_rx_stream_record_of) are a function of this record: 0-15 sample_his, 16-19 / 20-23 / 24-27 the windows, 28-30 their sums, 31 sense_count, 32 high_count,
 * 33 peak_corr, 34 peak_index, 35 update_cnt, 36 / 37 sum_dc re / im and 38 / 39 dc re / im, sign-extended (sora_amd.cs11a_record_words). */
typedef struct { sora_cca11a_state cca; sora_dcest11a_state dc; } sora_cs11a_state;
int sora_hip_carrier_sense11a(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, sora_cs11a_state* d_state, uint32_t* d_used, size_t nstreams,
                              size_t max_n, unsigned flags, void* stream);
/* T11aDataSymbol (PHY_11a.hpp:361-430), 80 -> 64: frame f owns d_nsym[f] symbols of 80 samples from SAMPLE d_first[f] of d_in (no alignment beyond a sample's); samples
 * 8..71 of symbol k (skip_cp = 8) go to SYMBOL d_out_first[f] + k of d_out, 64 samples each: the layout sora_hip_freq_comp11a / sora_hip_fft64 read.  The brick's
 * remain_symbols count-down and its Flush at zero are the host's.  max_nsym bounds every d_nsym[f]; at most 65535 frames per call. */
int sora_hip_data_symbol11a(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_nsym, const uint32_t* d_out_first, sora_complex16* d_out, size_t nframes,
                            size_t max_nsym, void* stream);
/* T11aViterbiSig (viterbi.hpp:8-49): d_soft[n][48] (sora_hip_deinterleave11a's output at n_bpsc 1) -> d_sig[n] = Viterbi_sig11's 24 decoded bits >> 6 */
int sora_hip_viterbi_sig11a(const uint8_t* d_soft, uint32_t* d_sig, size_t n, void* stream);
/* T11aPLCPParser (PHY_11a.hpp:518-604): d_sig[n] -> d_rec[n]: the context fields from 0 as the parser leaves them, with every reject of _parse_plcp in its order.  Reserved
 * bits (0xFC0010) or parity: nothing written.  Unknown rate code: data_rate_kbps written (0).  Length > 2500: data_rate_kbps, code_rate and frame_length written,
 * total_symbols not.  error_code is 0 or SORA_E_PLCP_HEADER_FAIL; total_symbols counts the SIGNAL symbol (remain_symbols starts from it). */
typedef struct { uint32_t error_code, data_rate_kbps, frame_length, code_rate, total_symbols; } sora_plcp11a_rec;
int sora_hip_plcp_parse11a(const uint32_t* d_sig, sora_plcp11a_rec* d_rec, size_t n, void* stream);

/* ---- The 40 MHz HT 2x2 receiver (sora_ht40_* below; parity unpinned, see there) as stages: the bricks of its data field and what its front end adds to the 802.11n stages.
 * With them every receive graph of the library stands as stages, and a host can replace ONE piece of this one -- its own detector in place of the unbiased MMSE, another
 * pilot tracker, its own noise estimate -- or compose the whole (sora_amd.rx_ht40_by_stages, rx_ht40_front_by_stages):
 *     downsample_ht40 -> the 802.11n stages cca11n .. sig_decode11n, the HT40 gate on the host | noise_var_ht40                              (front end: raw capture -> descriptor)
 *     freq_comp11n -> data_symbol_ht40 -> fft128 -> mimo_est_ht40                                                                           (HT-LTF 1 / 2)
 *     freq_comp11n -> data_symbol_ht40 -> fft128 -> mimo_comp_ht40 -> pilot_track_ht40        (symbol by symbol: theta of symbol d rotates symbol d + 1)
 *                  -> demap_ht40 -> deinterleave_ht40 (-> stream_join_ht40 in the joint coding) -> viterbi11n_ws -> desc11a -> frame_sink11a
 * A SHORT-GI frame (SORA_HT40_SHORT_GI on the descriptor's code rate; sora_ht40_set_guard below) is composed from the same stages, no new one: per data symbol d,
 * freq_comp11n over 18 bursts (144 samples) at offset + 320 + 144 d, then data_symbol_ht40 with first = offset + 320 + 144 d - 16, one symbol at a time -- the stage's samples
 * 32..159 are then exactly the symbol's 128 useful samples (sora_amd.rx_ht40_by_stages does this; tests/test_gpu_ht40_gi_stages.py holds it to the handle).
 * sora_hip_freq_comp11n with d_state[f] = { (n0 + k) cfo | 8 cfo | theta } is the 40 MHz frequency compensation of the burst that starts n0 samples into the frame.  The
 * conventions are those stated above sora_hip_cca11n: device pointers, stream order, no allocation, no host wait; a null pointer gives SORA_ERR_INVALID_PARAM before any device
 * work (sora_hip_last_error() names the function), a count of 0 is SORA_OK and launches nothing, no device SORA_ERR_NO_DEVICE.  The layouts are the handle's: weights and
 * channel matrix [frame][4][128] COMPLEX16 (entries 00, 01, 10, 11 per FFT bin), symbols [symbol][128].  Every stage equals tests/ht40_stage_model.py bit for bit
 * (tests/test_gpu_ht40_stages.py).  Buffers that are 16-byte (byte streams: 4-byte) aligned take the wide loads and stores; others work, more slowly.  DESIGN.md section 7, g1b. */
/* 2 x 160 -> 2 x 128, sora_hip_data_symbol11n at 40 MHz: frame f owns d_nsym[f] symbols of 160 samples from SAMPLE d_first[f] of both chains; samples 32..159 of symbol k go
 * to SYMBOL d_out_first[f] + k of d_out0 / d_out1, 128 samples each: the layout sora_hip_fft128 reads.  max_nsym >= every d_nsym[f]; at most 65535 frames per call. */
int sora_hip_data_symbol_ht40(const sora_complex16* d_in0, const sora_complex16* d_in1, const uint32_t* d_first, const uint32_t* d_nsym, const uint32_t* d_out_first,
                              sora_complex16* d_out0, sora_complex16* d_out1, size_t nframes, size_t max_nsym, void* stream);
/* d_ltf_r[f][256] = HT-LTF 1 | HT-LTF 2 of RX chain r after FFT<128>; d_noise_var[f] per carrier in LSB^2 of the FFT output, >= 0 (NULL: 0 for every frame).
 * d_h[f][4][128] (optional): TMimoChannelEst's P-matrix combination (p - q) / 2, (p + q) / 2 per chain, negated where the 40 MHz HT-LTF is -1.  d_w[f][4][128]: the
 * detection weights x 2^16 -- at noise_var 0 the brick's own 2x2 inverse (zero forcing), else the handle's unbiased MMSE W = diag((W' H)_ss)^-1 W', W' = (H^H H + s2 I)^-1 H^H
 * in single precision (+-1 LSB against a float64 evaluation), bit for bit what sora_ht40_process_dev exports as d_weights.  The 14 bins outside the 114 occupied carriers are 0
 * in both outputs (the handle leaves them meaningless). */
int sora_hip_mimo_est_ht40(const sora_complex16* d_ltf0, const sora_complex16* d_ltf1, const float* d_noise_var, sora_complex16* d_h, sora_complex16* d_w, size_t nframes,
                           void* stream);
/* TMimoChannelComp over 128 bins: x = sat((W y) >> 9); symbol s uses d_w[d_frame_index[s]] (NULL: frame 0); y_r = RX chain r after FFT<128>, x_k = spatial stream k */
int sora_hip_mimo_comp_ht40(const sora_complex16* d_w, const uint32_t* d_frame_index, const sora_complex16* d_y0, const sora_complex16* d_y1, sora_complex16* d_x0,
                            sora_complex16* d_x1, size_t nsym, void* stream);
/* The handle's pilot phase update: frame f owns symbols d_first[f] .. + d_nsym[f] - 1 of the two detected streams; per symbol theta += ((sum of stream 0's six dsp_atan16 at
 * bins -+53, -+25, -+11) / 6 + (stream 1's) / 6) >> 1, C division, every step through int16.  theta = vfo_theta_i[0..7] of d_state[f][24], the record sora_hip_freq_comp11n
 * reads: every entry takes the increments and is written back; the other sixteen words are not touched.  d_theta[s] (optional): vfo_theta_i[0] as it stands after symbol s. */
int sora_hip_pilot_track_ht40(const sora_complex16* d_x0, const sora_complex16* d_x1, const uint32_t* d_first, const uint32_t* d_nsym, int16_t* d_state, int16_t* d_theta,
                              size_t nframes, void* stream);
/* T11nDemap{BPSK,QPSK,QAM16,QAM64} over the 108 data carriers (-58..-2, 2..58 without the pilots): d_in[n][128] -> d_soft[n][108 N_BPSC] soft values 0..7, per carrier the I
 * bits then the Q bits.  n_bpsc 1, 2, 4 or 6, else SORA_ERR_INVALID_PARAM (so for the two stages below). */
int sora_hip_demap_ht40(const sora_complex16* d_in, uint8_t* d_soft, int n_bpsc, size_t n, void* stream);
/* The HT interleaver for 40 MHz (N_COL 18, N_ROW 6 N_BPSC, N_ROT 29) inverted: d_in / d_out [n][108 N_BPSC] of spatial stream 0 or 1 */
int sora_hip_deinterleave_ht40(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, int spatial_stream, size_t n, void* stream);
/* The joint coding's de-parser (TStreamJoin + TStreamConcat, sora_hip_stream_join11n at 108 carriers): two de-interleaved streams [n][108 N_BPSC] -> d_out[n][216 N_BPSC] in
 * groups of s = max(1, N_BPSC / 2) bytes alternating stream 0, stream 1: byte for byte one joint job's soft values for sora_hip_viterbi11n_ws. */
int sora_hip_stream_join_ht40(const uint8_t* d_s0, const uint8_t* d_s1, uint8_t* d_out, int n_bpsc, size_t n, void* stream);
/* The derotating decimator of the front end, both chains: stream f reads raw samples d_first[f] + 2 m, m = 0 .. d_n[f] - 1 (nothing behind the last of them), and writes kept
 * sample m at SAMPLE d_out_first[f] + m of d_out0 / d_out1: x[2m], negated with int16 saturation (-(-32768) = 32767) when d_m0[f] + m is odd.  d_m0[f] = the number (only its
 * parity counts) of the stream's first kept sample, so a stream cut into two calls gives what one call gives.  max_n bounds every d_n[f]; at most 65535 streams per call. */
int sora_hip_downsample_ht40(const sora_complex16* d_in0, const sora_complex16* d_in1, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_m0,
                             const uint32_t* d_out_first, sora_complex16* d_out0, sora_complex16* d_out1, size_t nstreams, size_t max_n, void* stream);
/* The front end's noise estimate: d_lltf_r[f][128] = the two L-LTF symbols of chain r after FFT<64> -> d_S[f] (optional) = the sum over both chains and the 52 occupied
 * carriers (bins 1..26, 38..63) of |Y1 - Y2|^2, an exact integer, and d_noise_var[f] = S / 416 rounded once to single precision. */
int sora_hip_noise_var_ht40(const sora_complex16* d_lltf0, const sora_complex16* d_lltf1, uint64_t* d_S, float* d_noise_var, size_t nframes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 802.11n 2x2 receive graph = CreateDemodGraph11n (kernel/bb/demod11/fb11ndemod_config.hpp:166-257) driven by
 * RxThread (kernel/bb/demod11/fb11n_demod.cpp:30-85) over a batch of independent captures of TWO RX chains at 40 MHz (the two
 * dump files Test11N_FB_Demod loads).  cfg->sample_rate_mhz must be 40; capture lengths are whole 28-sample source bursts; one
 * descriptor addresses the same range of both chain buffers.  Results as sora_rx_results reports them, with rate_kbps = the MCS
 * index (8..10: what the reference's SIG parser accepts), end_sample = the 40 MHz source position when RxThread sees the event,
 * start_sample / nsym / cfo_est 0.  A frame cut short by the end of its capture is decoded from zero-padded symbols, as the
 * reference's final flush does. */
typedef struct sora_rx11n sora_rx11n_t;
int   sora_rx11n_create(const sora_rx_cfg* cfg, sora_rx11n_t** out);
void  sora_rx11n_destroy(sora_rx11n_t* rx);
void* sora_rx11n_stream(sora_rx11n_t* rx);
int   sora_rx11n_process_dev(sora_rx11n_t* rx, const sora_complex16* d_iq0, const sora_complex16* d_iq1, const sora_capture_desc* caps, size_t ncaps);
int   sora_rx11n_process(sora_rx11n_t* rx, const sora_complex16* h_iq0, const sora_complex16* h_iq1, size_t nsamples_per_chain, const sora_capture_desc* caps, size_t ncaps);
int   sora_rx11n_results(sora_rx11n_t* rx, sora_frame_result* out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap);
/* Calls in flight, as for sora_rx_t: consecutive process calls rotate over `depth` pipelines (own stream and result arrays; default 1, at most 8), so
 * the latency-bound scan / symbol kernels of one call overlap the issue-bound trellis kernel of the call before it.  Every call has a ticket;
 * sora_rx11n_results / _stream refer to the most recent call, sora_rx11n_wait / _results_of to the call whose ticket is given (valid until `depth`
 * further calls have been made, or until the call is released: delivered and waited for, see sora_rx_wait_any); an input buffer must stay untouched until the call that reads it has
 * finished.  sora_rx11n_set_depth returns the
 * previous value (depth <= 0 only queries) and waits for the calls in flight; sora_rx11n_process (host buffers) also does. */
int   sora_rx11n_set_depth(sora_rx11n_t* rx, int depth);
/* As sora_rx_set_trellis, for T11aViterbi<..,192,36>: 64 = k_viterbi11n, 16 = k_viterbi16_11n, SORA_TRELLIS_WINDOWED = the frame's 192-bit trace-back windows decoded side
 * by side and proven afterwards (k_viterbi16w_11n + k_win_redo_11n: bit-exact by construction like the 802.11a form; new in ABI 4), 0 (default since ABI 4; it was 64) =
 * chosen by the library: window-parallel while depth x max_captures x max_frames_per_capture <= 2048 (a frame per wave-slot leaves the chip idle: a lone capture's
 * frame), k_viterbi11n above that.  Returns the previous setting, a negative argument only queries; sora_rx11n_trellis resolves the automatic choice;
 * sora_rx11n_window_stats is sora_rx_window_stats for this handle. */
int   sora_rx11n_set_trellis(sora_rx11n_t* rx, int lanes_per_pair);
int   sora_rx11n_trellis(sora_rx11n_t* rx);
int   sora_rx11n_window_stats(sora_rx11n_t* rx, unsigned long long out[4]);
/* Highest MCS the handle's SIG parser accepts: 10 (default: exactly PHY_11n.hpp:497) .. 14.  Returns the previous value; <= 0 only queries; any other value:
 * SORA_ERR_INVALID_PARAM.  Waits for the calls in flight and re-sizes the pipelines (SORA_ERR_CAPACITY, and no change, where max_total_samples does not fit the wider
 * symbol slots of one handle); in stream mode it starts every stream afresh.
 *   - The reference's behaviour: everything at the default.  With the gate at 10 every row, byte and position is what the reference's graph gives; MCS 11..14 frames
 *     are PLCP header failures, as T11nSigParser::_parse_htsig reports them (ht_frame_mcs >= 11).
 *   - The library's own definition, with the gate raised: "the reference's graph with the one comparison moved".  CreateDemodGraph11n is wired for these rates --
 *     rate_selector routes MCS 11/12 to T11nDemapQAM16 -> T11nDeinterleaveQAM16_S0/_S1 -> TStreamJoin<2,208> -> TStreamConcat<2,2> and MCS 13/14 to the QAM64 bricks
 *     -> TStreamJoin<2,312> -> TStreamConcat<2,3>, all into the one T11aViterbi<5000*8,312,192,36> (rate 1/2 for MCS 11, 3/4 for 12 and 14, 2/3 for 13) -- and
 *     this handle runs those bricks; the symbol count follows N_DBPS = 208, 312, 416, 468.  No compiled reference decodes such a frame: tests/rx11n_ext_model.py
 *     restates that graph from the reference-pinned stage functions and is what the GPU rows are compared with.  rate_kbps carries the MCS index 11..14.
 *   - Unchanged at every gate: MCS < 8 and MCS 15 are refused, as are HT lengths above 1500 and every L-SIG check. */
int   sora_rx11n_set_mcs_max(sora_rx11n_t* rx, int mcs_max);
int   sora_rx11n_ticket(sora_rx11n_t* rx);
int   sora_rx11n_synchronize(sora_rx11n_t* rx);                                                       /* every call issued so far has finished */
int   sora_rx11n_wait(sora_rx11n_t* rx, int ticket);
/* as sora_rx_wait_any: the oldest FINISHED call with an enqueued delivery; it is then released and its pipeline reused first */
int   sora_rx11n_wait_any(sora_rx11n_t* rx, int* ticket);
int   sora_rx11n_results_of(sora_rx11n_t* rx, int ticket, sora_frame_result* out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap);
/* as sora_rx11b_deliver_async */
int   sora_rx11n_deliver_async(sora_rx11n_t* rx, int ticket, sora_frame_result* h_rows, size_t max_rows, uint32_t* h_counts, uint8_t* h_mpdu, size_t mpdu_cap);
/* Stream continuation, as sora_rx11b_set_stream_mode (the live-source case: a host binds CreateDemodGraph11n to TRxStream, and the graph's
 * carrier-sense state -- the two chains' MimoAutoCorr rings and running sums, the delayed-energy ring, the TCCA11n counters -- carries over from
 * one read to the next).  With sora_rx11n_set_stream_mode(rx, 1) capture k of a process call CONTINUES capture k of the call before it; one
 * descriptor addresses the same range of both chain buffers, as in every call:
 *   - after a call, sora_rx11n_stream_consumed(rx, ticket, h, n) gives, per capture, the RESUME POINT: the number of 40 MHz samples of that
 *     capture that are final.  It is a position where a 4-sample burst boundary of the 20 MHz graph falls on a source-call boundary (14
 *     samples at 20 MHz, 28 at 40 MHz) while the graph is in carrier sense; bursts restart at each post-event origin, which is a call
 *     boundary, so it is a multiple of 28 (0 if the capture holds none).  Every row the call reports ends at or in front of it
 *     (end_sample <= resume point);
 *   - NO FLUSH: stream mode never issues the end-of-stream flush that ends a capture with the mode off (TMemSamples2 running dry: missing
 *     symbols read as zeros).  A capture's end is not the stream's end, so a frame still running when the capture ends -- its L-LTF, SIG,
 *     HT-LTF or data symbols reach past the capture -- lies behind the resume point and is NOT reported, nor decoded from zero padding: the
 *     next call finds it again, so every frame is reported exactly once.  When a capture holds more row events than max_frames_per_capture,
 *     its resume point stops in front of the first event that found no row: no event is lost.  A zero-length capture leaves its stream as
 *     it was;
 *   - the host builds the next call's capture k from the stream FROM THAT POINT on: the unconsumed tail of what it submitted plus whatever
 *     has arrived since, in both chains (capture lengths are still whole 28-sample source calls).  The library starts it with the state the
 *     graph had at the resume point, so the rows of all the calls together (positions relative to their own capture: add the stream position
 *     of its first sample) are exactly the events RxThread reports on the uncut stream -- tests/test_gpu_stream11n.py holds streams cut at
 *     random source calls to the compiled reference graph's events on the whole;
 *   - calls of a handle in stream mode run one after the other (a process call first waits for every call in flight: it needs their
 *     records); throughput comes from many streams (captures) per call.  Both process forms, every trellis choice and any depth work in stream
 *     mode: the records belong to the handle, not to a pipeline.  sora_rx11n_stream_consumed exists for the most recent ticket only.
 *     Switching the mode, either way, starts every stream afresh.
 * Returns the previous mode; a negative argument only queries. */
int   sora_rx11n_set_stream_mode(sora_rx11n_t* rx, int enable);
int   sora_rx11n_stream_consumed(sora_rx11n_t* rx, int ticket, uint32_t* h_consumed, size_t ncaps);

/* ------------------------------------------------------------------------------------------------
 * The data field of an HT-mixed 40 MHz, two-stream frame (BASELINE.json configs[3]: 128-point FFT, MMSE MIMO detection, one decoder per
 * spatial stream).  PARITY UNPINNED: the reference has no such graph (its 802.11n receiver is 20 MHz, zero-forcing, one decoder, MCS 8-10:
 * kernel/bb/Brick11/src/PHY_11n.hpp:497, channel_11n.hpp:423-433); every brick it does have is used with the reference's arithmetic
 * (FFT<128>, TFreqComp_11n, TMimoChannelEst / TMimoChannelComp -- noise_var = 0 gives exactly their zero-forcing weights --, TPilotTrack_11n,
 * T11nDemap*, T11aViterbi<..,192,36>, T11aDesc, CRC-32), the 40 MHz carrier plan / HT-LTF / interleaver come from IEEE 802.11n-2009 and
 * are modelled independently in oracle/py_ht40.py.  The caller supplies what the (20 MHz, reference-pinned) front end finds: where the first
 * HT-LTF symbol starts, modulation, code rate, PSDU lengths, CFO.  A frame = 2 HT-LTF symbols + nsym data symbols of 160 samples at 40 MHz on
 * two RX chains; each spatial stream carries its own PSDU (SERVICE + PSDU incl. FCS + tail, scrambled, K = 7 coded, punctured, interleaved).
 * Results: two rows per frame (start_sample = spatial stream 0 / 1, error_code FRAME_OK / CRC32_FAIL, length, crc32, nsym;
 * rate_kbps = 10 n_bpsc + code_rate); d_weights (optional, [nframes][4][128] COMPLEX16) receives the detection weights x 2^16.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    uint64_t offset;        /* 40 MHz samples from both iq bases to the first sample (cyclic prefix) of HT-LTF 1 */
    uint32_t n_bpsc;        /* 1, 2, 4, 6 */
    uint32_t code_rate;     /* SORA_CR_12 / _23 / _34 */
    uint32_t length[2];     /* PSDU bytes (FCS included) of spatial stream 0 / 1, <= 4000 */
    int32_t  cfo;           /* phase step per 40 MHz sample, 65536 = 2 pi (TFreqComp_11n: the running phase is n * cfo - theta) */
    float    noise_var;     /* noise variance per carrier in LSB^2 of the FFT<128> output; 0 = zero forcing; > 0: unbiased MMSE,
                             * W = diag((W'H)_ss)^-1 W', W' = (H^H H + noise_var I)^-1 H^H */
    uint32_t frame_id;      /* echoed into the rows' capture_id */
} sora_ht40_frame;
typedef struct sora_ht40 sora_ht40_t;
uint32_t sora_ht40_symbols(uint32_t length0, uint32_t length1, uint32_t n_bpsc, uint32_t code_rate);   /* data symbols of such a frame (0: bad arguments) */
/* max_soft_values >= sum over frames of 2 x nsym x 108 n_bpsc (+ 64 per frame) */
int   sora_ht40_create(int device, uint32_t max_frames, uint64_t max_soft_values, sora_ht40_t** out);
void  sora_ht40_destroy(sora_ht40_t* rx);
void* sora_ht40_stream(sora_ht40_t* rx);                                                               /* the stream of the most recent process call */
/* 16 (default: the handle keeps eight calls in flight) / 64: as sora_rx_set_trellis (the two streams of a frame are one pair) */
int   sora_ht40_set_trellis(sora_ht40_t* rx, int lanes_per_pair);
int   sora_ht40_synchronize(sora_ht40_t* rx);                                                          /* every call issued so far has finished (a handle keeps eight calls in flight:
                                                                                                        * process_dev waits only for the call eight calls back; results reports the most recent one) */
int   sora_ht40_process_dev(sora_ht40_t* rx, const sora_complex16* d_iq0, const sora_complex16* d_iq1, const sora_ht40_frame* h_frames, size_t nframes, sora_complex16* d_weights);
int   sora_ht40_results(sora_ht40_t* rx, sora_frame_result* h_out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap);
/* Diagnostic, for tests (like d_weights): the nsym x 108 x n_bpsc de-interleaved soft bytes (0..7 each, one per coded bit, as the trellis reads them) of spatial
 * stream `stream` (0 / 1) of described frame `frame` of the sora_ht40_process_dev call `ticket`.  Waits for that call as sora_ht40_results_of does.  *nsoft receives
 * the count, also when cap is too small (SORA_ERR_CAPACITY; nothing is copied then).  SORA_ERR_INVALID_PARAM: a stale ticket, a raw-capture call (its frames are
 * planned on the device), no such frame or stream.  tests/test_gpu_ht40_soft.py holds these bytes, bit for bit, to oracle/ht40_data_model.py. */
int   sora_ht40_soft_of(sora_ht40_t* rx, int ticket, uint32_t frame, uint32_t stream, uint8_t* h_soft, size_t cap, size_t* nsoft);
/* The same receiver on RAW CAPTURES, as every other handle takes its input: two-chain 40 MHz captures (whole 28-sample source bursts,
 * offsets a multiple of 4) in, the front end finds the frames.  The legacy preamble and HT-SIG of an HT-mixed 40 MHz frame are the 20 MHz
 * waveforms sent on both halves of the channel (the upper one rotated by 90 degrees), so the even samples of x[n] j^n are (1 + j) times
 * the 20 MHz legacy waveform and the reference's own bricks apply unchanged: TCCA11n (cca_11n.hpp:5-171), the L-LTF frequency offset
 * (freqoffset_11n.hpp:86-280), TSisoChannelEst / Comp, T11nSigDemap, the SIG decoder and T11nSigParser (PHY_11n.hpp:400-514) with one
 * gate relaxed -- MCS 8..14 at CBW 40 and LENGTH <= 4000 are accepted where PHY_11n.hpp:497-505 accepts MCS 8..10 and 1500.  Own
 * definitions (parity unpinned): each spatial stream carries its own PSDU of HT-SIG's LENGTH through its own encoder (configs[3]'s
 * "dual Viterbi"), the CFO handed to the data field is the L-LTF estimate, the noise variance the MMSE detector uses is estimated from
 * the difference of the two L-LTF symbols.  Rows: per event in (capture, time) order; a recorded frame reports two rows (start_sample =
 * spatial stream, rate_kbps = MCS, end_sample = 40 MHz source position of the event, FRAME_OK / CRC32_FAIL), a header that fails one row
 * (SORA_E_PLCP_HEADER_FAIL); a frame the capture cuts off raises no event.  Tickets / results_of / deliver_async as above.  The call is one
 * chain of kernels (the front end's records become the data field's tables on the device, k_ht40_plan): no host wait inside it; captures that
 * hold more frames / soft values than the handle was created for are reported by sora_ht40_wait / _results_of (SORA_ERR_CAPACITY). */
int   sora_ht40_process_captures_dev(sora_ht40_t* rx, const sora_complex16* d_iq0, const sora_complex16* d_iq1, const sora_capture_desc* h_caps, size_t ncaps,
                                     uint32_t max_frames_per_capture);
/* The front end's own definitions, stated in full (tests/cxx/ht40_front_model.c restates them on the oracle's bricks and tests/test_gpu_ht40_front.py holds the
 * records below to that model, field for field):
 *   - kept sample m of a capture (m counts from the capture's first sample, and on from call to call in stream mode) is x[2m], negated with int16 saturation
 *     when m is odd (-(-32768) = 32767);
 *   - the gate behind T11nSigParser's own checks (L-SIG tail / reserved bit / parity / rate, HT-SIG CRC-8 and tail) is 8 <= MCS <= 14 && CBW 40 && 4 <= LENGTH <= 4000;
 *     the parser's L-SIG bound (2 x the L-SIG LENGTH field <= 1500, PHY_11n.hpp _parse_plcp) stands as it is, so a frame that announces more than 750 there
 *     -- about 1 ms behind L-SIG: MCS 8 beyond roughly 1650 bytes -- fails its header whatever HT-SIG says;
 *   - a frame with a sound header is an event only if HT-STF, both HT-LTFs and all nsym data symbols lie inside the capture's real samples (nsym =
 *     sora_ht40_symbols, in joint coding sora_ht40_symbols_joint); otherwise there is no event and the capture is over.  A capture that ends inside the SIG field
 *     decodes its missing symbols as zeros, as the reference's flush does: a header that fails then is an event, one that passes is a frame cut off;
 *   - end_sample and the origin of the next carrier sense follow RxThread's source calls of 28 samples;
 *   - noise_var = S / 416 in single precision, S = the sum of |Y1 - Y2|^2 over the 52 occupied carriers of both chains' two L-LTF FFT<64> outputs.
 * Diagnostic, for tests (like sora_ht40_soft_of: no kernel and no launch differ for it): the records of capture `capture` (index into the call's h_caps) of the
 * raw-capture call `ticket`, in time order.  Waits for that call as sora_ht40_results_of does, and answers also for a call that ended in SORA_ERR_CAPACITY (the
 * records exist either way).  *nfound receives min(events the capture raised, max_frames_per_capture), also when cap is too small (SORA_ERR_CAPACITY; nothing is
 * copied then).  SORA_ERR_INVALID_PARAM: a stale ticket, a descriptor call, a capture index past the call's. */
typedef struct {
    uint32_t a20;           /* 20 MHz index in the capture (40 MHz sample 2 x a20) behind the last SIG symbol taken: the first HT-STF sample of a recorded frame */
    uint32_t mcs, ht_len;   /* HT-SIG's MCS and LENGTH; 0 unless the frame was recorded */
    uint32_t nsym;          /* data symbols in the call's coding; 0 unless the frame was recorded */
    int32_t  cfo;           /* the L-LTF estimate, phase step per 20 MHz sample, 65536 = 2 pi; the data field takes cfo / 2 (C division: toward zero) */
    float    noise_var;     /* as handed to the data field */
    uint32_t end_sample;    /* 40 MHz source position at which the event is seen */
    uint32_t error_code;    /* 0: recorded (the data field's rows say FRAME_OK / CRC32_FAIL), else SORA_E_PLCP_HEADER_FAIL */
} sora_ht40_found;
int   sora_ht40_found_of(sora_ht40_t* rx, int ticket, uint32_t capture, sora_ht40_found* h_found, size_t cap, size_t* nfound);
/* Tickets, as for sora_rx_t: every process call has one; it stays valid until sora_ht40_calls_in_flight() (8) further calls have reused its
 * slot (or, once the call is released -- delivered and waited for -- until the next call, which takes a released slot first) -- so back-to-back calls are all collectable, each by its own
 * ticket, while later ones run.  The INPUT buffers of a call must stay
 * untouched until sora_ht40_wait(its ticket) (or _results_of, or _synchronize) has returned. */
int   sora_ht40_ticket(sora_ht40_t* rx);                       /* ticket of the most recent process call (0: none) */
int   sora_ht40_calls_in_flight(sora_ht40_t* rx);              /* how many calls the handle keeps addressable */
int   sora_ht40_wait(sora_ht40_t* rx, int ticket);
/* as sora_rx_wait_any: the oldest FINISHED call with an enqueued delivery; it is released and its slot reused first */
int   sora_ht40_wait_any(sora_ht40_t* rx, int* ticket);
void* sora_ht40_stream_of(sora_ht40_t* rx, int ticket);
int   sora_ht40_results_of(sora_ht40_t* rx, int ticket, sora_frame_result* h_out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap);
/* As sora_rx11b_deliver_async.  The delivered table is the one sora_ht40_results_of reports, in (capture, time) order: two rows per RECORDED frame
 * (one per spatial stream, start_sample = the stream) and -- raw-capture calls -- one row per event that ended in the front end (an HT-SIG whose CRC-8
 * fails, an unsupported MCS: E_ERROR_PLCP_HEADER_FAIL, no PSDU); the rows of the last event a full capture could hold carry SORA_ROW_TRUNCATED.
 * max_rows: at least 2 x the call's frames (descriptor calls) / 2 x ncaps x max_frames_per_capture (raw-capture calls: the host knows only that bound). */
int   sora_ht40_deliver_async(sora_ht40_t* rx, int ticket, sora_frame_result* h_rows, size_t max_rows, uint32_t* h_counts, uint8_t* h_mpdu, size_t mpdu_cap);
/* Stream continuation of the raw-capture form, as sora_rx11n_set_stream_mode (the live-source case: a host with a two-chain 40 MHz source hands
 * the stream over in pieces, and the front end's carrier-sense state -- the two chains' MimoAutoCorr rings and running sums, the delayed-energy
 * ring, the TCCA11n counters -- carries over from one read to the next).  With sora_ht40_set_stream_mode(rx, 1) capture k of a
 * sora_ht40_process_captures_dev call CONTINUES capture k of the previous such call; one descriptor addresses the same range of both chain
 * buffers, as in every call:
 *   - after a call, sora_ht40_stream_consumed(rx, ticket, h, n) gives, per capture, the RESUME POINT: the number of 40 MHz samples of that
 *     capture that are final.  It is a position where a 4-sample burst boundary of the 20 MHz front end falls on a source-call boundary (14
 *     samples at 20 MHz, 28 at 40 MHz) while the front end is in carrier sense; bursts restart at each post-event origin, which is a call
 *     boundary, so it is a multiple of 28 (0 if the capture holds none).  Every row the call reports ends at or in front of it
 *     (end_sample <= resume point).  (A multiple of 28 is an even number of 20 MHz samples: the front end's derotation x[2m] (-1)^m runs on
 *     unbroken, so the 40 MHz handle needs no alignment rule beyond "continue from the resume point".);
 *   - NO PADDING: with the mode off a capture's last burst is delivered zero-padded and missing SIG symbols read as zeros; stream mode never
 *     reads zeros past the capture's end.  A frame is taken only when its L-LTF, its three SIG symbols and -- for a valid header -- its
 *     HT-STF, both HT-LTFs and all data symbols lie inside the capture's samples; otherwise the capture ends at the latest resume point in
 *     front of the frame's detection and the next call finds the frame again, so every frame is reported exactly once.  A header that fails
 *     with its three SIG symbols inside the capture is an event as usual.  An event that finds no row slot (max_frames_per_capture) stops
 *     the capture's resume point in front of it: no event is lost.  A zero-length capture leaves its stream as it was;
 *   - the host builds the next call's capture k from the stream FROM THAT POINT on: the unconsumed tail of what it submitted plus whatever
 *     has arrived since, in both chains (capture lengths are still whole 28-sample source bursts).  The library starts it with the state
 *     the front end had at the resume point, so the rows of all the calls together (positions relative to their own capture: add the stream
 *     position of its first sample) are exactly the rows the mode-off handle reports on the uncut stream -- tests/test_gpu_stream_ht40.py
 *     holds streams cut at random source calls to that;
 *   - calls of a handle in stream mode run one after the other (a sora_ht40_process_captures_dev call first waits for every call of the
 *     handle in flight: it needs their records); throughput comes from many streams (captures) per call.  Both trellis choices work in
 *     stream mode: the records belong to the handle, not to a slot.  sora_ht40_stream_consumed exists for the most recent ticket only.
 *     Switching the mode, either way, first waits for every call in flight and starts every stream afresh.  sora_ht40_process_dev (the
 *     descriptor form) does not touch the records;
 *   - sora_ht40_create takes no capture count: the records are sized once, when the mode is first enabled, for max_frames streams, and a
 *     raw-capture call in stream mode with ncaps > max_frames answers SORA_ERR_INVALID_PARAM before anything is launched;
 *   - a stream-mode call that ends in SORA_ERR_CAPACITY (more frames / soft values than the handle was created for) has already advanced
 *     its streams: its frames are lost, nothing is rolled back, and the host restarts the streams by switching the mode.
 * sora_ht40_set_stream_mode returns the previous mode; a negative argument only queries.  sora_ht40_stream_consumed fails when the handle
 * is not in stream mode (SORA_ERR_FAILED), for any ticket but the most recent call's and for more captures than that call had
 * (SORA_ERR_INVALID_PARAM). */
int   sora_ht40_set_stream_mode(sora_ht40_t* rx, int enable);
int   sora_ht40_stream_consumed(sora_ht40_t* rx, int ticket, uint32_t* h_consumed, size_t ncaps);
/* The handle's CODING.  SORA_HT40_CODING_PER_STREAM (the default) is everything above: two PSDUs of equal length per frame, one decoder per spatial stream.
 * SORA_HT40_CODING_JOINT takes the frames of sora_hip_tx_ht40_joint (its comment states the format): ONE PSDU per frame, one encoder's output stream-parsed over the
 * two streams, one decoder.  HT-SIG does not signal the coding; the handle's setting decides.  A handle in joint coding:
 *   - descriptor calls: length[0] is the PSDU length and length[1] must be 0 (else SORA_ERR_INVALID_PARAM before anything is launched); nsym =
 *     sora_ht40_symbols_joint(length[0], n_bpsc, code_rate); ONE row per frame: start_sample 0, error_code, length, crc32, nsym and rate_kbps as above, capture_id =
 *     frame_id.  max_soft_values: the same rule (a frame holds the same number of soft bytes);
 *   - raw-capture calls and stream mode work as above with ONE row per recorded frame; a frame's extent follows the joint N_SYM;
 *   - sora_ht40_soft_of: `stream` must be 0; the 2 x nsym x 108 x n_bpsc MERGED soft bytes are returned, as the trellis reads them (symbol after symbol, the
 *     symbol's 2 N_CBPSS coded bits in the encoder's order);
 *   - sora_ht40_deliver_async: raw-capture calls take max_rows as above (the bound is not halved: the event table keeps its two-row pitch); descriptor calls
 *     need one row per frame.
 * Returns the previous value; a negative argument only queries.  Like sora_ht40_set_stream_mode it first waits for every call in flight and starts every stream
 * afresh.  Calls issued before the switch keep their coding when their results are read. */
#define SORA_HT40_CODING_PER_STREAM 0
#define SORA_HT40_CODING_JOINT      1
int      sora_ht40_set_coding(sora_ht40_t* rx, int coding);
uint32_t sora_ht40_symbols_joint(uint32_t length, uint32_t n_bpsc, uint32_t code_rate);   /* data symbols of a joint-coded frame (0: bad arguments) */
/* The SHORT GUARD INTERVAL (opt-in; sora_hip_tx_ht40_gi states the format; DESIGN.md section 7 "g4").  A short-GI frame has the same N_SYM and the same soft bytes as
 * the long-GI frame of its PSDUs; only the data symbols lie elsewhere: symbol d starts 320 + 144 d samples behind `offset` and its 128 useful samples 16 further on (long:
 * 320 + 160 d, 32).  The compensation phase stays n cfo - theta with n the sample's index in the frame.
 *   - descriptor calls: sora_ht40_frame.code_rate may carry SORA_HT40_SHORT_GI OR-ed onto SORA_CR_*; the frame is then 2 HT-LTF symbols of 160 samples plus nsym data
 *     symbols of 144 samples from `offset`.  Any other bit above the SORA_CR_* value stays SORA_ERR_INVALID_PARAM.  This works whatever the handle's guard mode is, in
 *     both codings, and long and short frames may share a call;
 *   - raw captures: sora_ht40_set_guard(rx, SORA_HT40_GUARD_SIGNALLED) makes the front end read HT-SIG bit 31 (Short GI; its CRC-8 covers it).  A frame with a sound
 *     header and the bit set occupies 20 MHz samples [a, a + 240 + 72 nsym) from its first HT-STF sample a, and is an event only if all of that lies inside the
 *     capture's real samples; end_sample and the origin of the next carrier sense follow the source-call rule above from that end, and the data field takes the short
 *     geometry from `offset` = capture + 2 a20 + 160 + 16: the front end's a20 lies 21..28 samples in front of the frame's own timing -- inside a 32-sample guard
 *     interval, in front of a 16-sample one -- so a short-GI frame is taken 16 samples later, HT-LTFs and data alike, which puts every window 5..12 samples inside
 *     its prefix (fewer than 16 where the capture ends inside them: as far as its samples reach; such a capture cuts the frame's own tail).  A frame with the bit
 *     clear is handled exactly as in SORA_HT40_GUARD_LONG (the default), where the bit is not looked at: a short-GI frame is then cut at the long
 *     positions and reported CRC32_FAIL, as before.  Works in both codings and in stream mode (a short-GI frame that runs past the piece is found by the next call,
 *     as a long one is -- it is taken once those 16 samples behind its extent lie inside the piece too, so that every cut gives the one-call result;
 *     sora_ht40_stream_consumed means what it meant);
 *   - results: the rows of a short-GI frame carry SORA_ROW_SHORT_GI in flags (beside SORA_ROW_TRUNCATED where that applies) -- both rows of a per-stream frame, the one
 *     row of a joint frame, in both call forms and through sora_ht40_deliver_async; rate_kbps is unchanged.  sora_ht40_found.mcs carries SORA_HT40_SHORT_GI OR-ed onto the
 *     MCS of a recorded short-GI frame.  sora_ht40_soft_of, d_weights and max_soft_values are unchanged.
 * Calls that cannot hold a short frame -- descriptor calls without the flag, raw-capture calls of a handle in SORA_HT40_GUARD_LONG -- launch the kernels they always
 * launched.  sora_ht40_set_guard returns the previous mode; a negative argument only queries.  Like sora_ht40_set_coding it first waits for every call in flight and
 * starts every stream afresh; calls issued before the switch keep their mode when their results are read.  The 20 MHz 802.11n pair has no short GI. */
#define SORA_HT40_SHORT_GI        0x100u  /* on sora_ht40_frame.code_rate (in) and sora_ht40_found.mcs (out) */
#define SORA_HT40_GUARD_LONG      0
#define SORA_HT40_GUARD_SIGNALLED 1
int      sora_ht40_set_guard(sora_ht40_t* rx, int mode);

/* MCS 15 (two streams, 64-QAM, rate 5/6; 270 / 300 Mbit/s with the long / short guard interval) on the receive handle.  The rate's
 * definition -- the puncture pattern and the decoder -- is SORA_CR_56's and sora_hip_viterbi56_11n's above: N_CBPS per stream is 108 N_BPSC, a whole number of 6-value
 * groups for every N_BPSC; N_DBPS is 90 N_BPSC per stream (540 at MCS 15) and twice that in the joint coding (1080).
 * sora_ht40_set_mcs_max(rx, mcs_max) sets the gate: 14 (the default) or 15, anything else above 0 is SORA_ERR_INVALID_PARAM; returns the previous value; an argument
 * <= 0 only queries.  Like sora_ht40_set_guard it first waits for every call in flight and starts every stream afresh (a frame the gate now admits changes what a
 * stream holds).  With the gate at 14 nothing differs: SORA_CR_56 on a descriptor is SORA_ERR_INVALID_PARAM, MCS 15 in HT-SIG is a header failure, every call launches
 * the kernels it always launched.  With the gate at 15:
 *   - descriptor calls: sora_ht40_frame.code_rate may be SORA_CR_56, with or without SORA_HT40_SHORT_GI, with any n_bpsc of 1 / 2 / 4 / 6, in both codings; rows of such a
 *     frame carry rate_kbps = 10 n_bpsc + 3.  sora_ht40_soft_of works unchanged (the soft bytes do not depend on the code rate).
 *   - raw captures: the front end's gate is 8 <= MCS <= 15; a recorded MCS 15 frame has sora_ht40_found.mcs = 15 and rows with rate_kbps = 15.
 *   - the frames of rate 5/6 are a FOURTH job list, decoded by k_viterbi56_11n behind the call's trellis kernel: launched for a descriptor call only when the call
 *     holds such a frame, for a raw-capture or stream-mode call always (on an empty list its waves return at once).  sora_ht40_set_trellis does not apply to that
 *     list: it has one kernel, 64 lanes per pair -- the two streams of a frame, or two joint frames.
 * sora_ht40_symbols accepts code_rate SORA_CR_56 whatever a handle's gate is (a pure function); sora_ht40_symbols_joint keeps answering it with 0, as it always has (a
 * test of the joint coding pins that): a joint rate-5/6 frame has ceil((16 + 8 LENGTH + 6) / (180 N_BPSC)) data symbols, and a gate-15 handle's rows report the count.
 * Not offered: MCS 15 on the 20 MHz pair (sora_rx11n_*, sora_hip_tx11n: its symbol-slot storage is sized for 3/4), the stage compositions at rate 5/6, BRICK adapters,
 * the sixteen-lane and window-parallel trellis forms for rate 5/6. */
int      sora_ht40_set_mcs_max(sora_ht40_t* rx, int mcs_max);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU sharding for a C host.  Captures are independent -- the reference resets its context per
 * frame (kernel/bb/demod11/fb11ademod_config.hpp:68-95) and RxThread walks one dump at a time (fb11a_demod.cpp:29-81) -- so
 * rank r of W runs sora_rx_* on its own block of captures in its own HBM (sora_shard_partition) and nothing is exchanged on
 * the data path.  These calls are the result exchange: ncclAllGather of the dense 36-byte result rows and of the per-rank row
 * counts, ncclAllReduce(sum) of counters, on RCCL over xGMI, one process per GPU.  The 128-byte id is made on rank 0 and
 * carried to the other ranks by the host (file, socket, MPI ...).  RCCL is loaded on the first sora_shard_* call.
 *   sora_shard_gather_rows     device buffers, asynchronous on `stream`: d_rows must hold max_rows_per_rank rows (rows past
 *                              *d_nrows are padding), d_all_rows world x max_rows_per_rank rows, d_all_counts world counts
 *   sora_shard_gather_results  convenience for sora_rx_t: the rows of a finished process call (ticket, or 0 = the most recent)
 *                              of every rank, compacted in rank order into h_all_rows (world x max_rows_per_rank rows of room),
 *                              h_counts[world], *n_total; blocks until done.  capture_id is the caller's own numbering, so a
 *                              host that numbers captures globally gets a table it can use as it is.
 * ------------------------------------------------------------------------------------------------ */
#define SORA_SHARD_ID_BYTES 128
typedef struct sora_shard sora_shard_t;
int  sora_shard_unique_id(uint8_t id[SORA_SHARD_ID_BYTES]);
int  sora_shard_create(const uint8_t id[SORA_SHARD_ID_BYTES], int world_size, int rank, int device, sora_shard_t** out);
void sora_shard_destroy(sora_shard_t* sh);
int  sora_shard_world(const sora_shard_t* sh, int* world_size, int* rank);
void sora_shard_partition(size_t n_items, int world_size, int rank, size_t* first, size_t* count);
int  sora_shard_gather_rows(sora_shard_t* sh, const sora_frame_result* d_rows, const uint32_t* d_nrows, size_t max_rows_per_rank,
                            sora_frame_result* d_all_rows, uint32_t* d_all_counts, void* stream);
int  sora_shard_reduce_counters(sora_shard_t* sh, uint64_t* d_counters, size_t n, void* stream);
int  sora_shard_gather_results(sora_shard_t* sh, sora_rx_t* rx, int ticket, size_t max_rows_per_rank,
                               sora_frame_result* h_all_rows, uint32_t* h_counts, size_t* n_total);
/* The same with the MPDUs (what fb11a_demod.cpp:64-70 hands to the MAC): every rank's MPDU bytes, densely packed in row order, gathered
 * with one more ncclAllGather of max_mpdu_bytes_per_rank bytes per rank; the gathered rows' mpdu_offset indexes h_all_mpdu
 * (world x max_mpdu_bytes_per_rank bytes of room), *mpdu_total = bytes used.  h_all_mpdu = NULL: rows only.
 * Every rank must make the call (three collectives); a rank whose own part fails still takes part and every rank then returns an error. */
int  sora_shard_gather_results_mpdu(sora_shard_t* sh, sora_rx_t* rx, int ticket, size_t max_rows_per_rank, sora_frame_result* h_all_rows,
                                    uint32_t* h_counts, size_t* n_total, size_t max_mpdu_bytes_per_rank, uint8_t* h_all_mpdu, size_t* mpdu_total);

/* ------------------------------------------------------------------------------------------------
 * 802.11b receive graph = CreateDemodGraph (kernel/bb/demod11/fb11bdemod_config.hpp:122-172) driven by
 * MAC11b_Receive (kernel/bb/demod11/fb11b_demod.cpp:27-76) over a batch of independent 44 MHz captures: TDCRemove,
 * TEnergyDetect / TDCEstimator, TSymTiming, TBarkerSync, TBB11bDespread, TSFDSync, TDBPSKDemap / TDQPSKDemap,
 * TCCK5P5Decoder / TCCK11Decoder (kernel/bb/Brick11/src/cck.hpp), TDesc741, TBB11bPlcpParser, TBB11bFrameSink.  cfg->sample_rate_mhz must be 44; capture lengths are whole 28-sample bursts.
 * Result rows: end_sample = CF_MemSamples::mem_sample_index() when the harness sees the event (44 MHz samples);
 * error_code also takes SORA_E_SFD_FAIL / SORA_E_SFD_TIMEOUT / SORA_E_SYNC_TIMEOUT; crc32 = the reference's FCS word (three
 * FCS bytes and one stale buffer byte, PHY_11b.hpp:725-731); start_sample, nsym and cfo_est are 0.  Long preamble (the short one too with
 * sora_rx11b_set_preamble); 1 Mbps DBPSK, 2 Mbps DQPSK, 5.5 and 11 Mbps CCK payloads (all four rates of the reference graph).
 * Two kernels per call: the first has no CCK decoders in it (more resident waves) and hands a capture over when a header announces
 * 5.5 / 11 Mbps; the second redoes the handed-over captures.
 * ------------------------------------------------------------------------------------------------ */
#define SORA_E_NOT_SUPPORTED     ((int)0x80000003)
#define SORA_E_SFD_FAIL          ((int)0x80000004)
#define SORA_E_SFD_TIMEOUT       ((int)0x80000008)
#define SORA_E_SYNC_TIMEOUT      ((int)0x80000009)
typedef struct sora_rx11b sora_rx11b_t;
int  sora_rx11b_create(const sora_rx_cfg* cfg, sora_rx11b_t** out);
void sora_rx11b_destroy(sora_rx11b_t* rx);
void* sora_rx11b_stream(sora_rx11b_t* rx);            /* the HIP stream of the most recent process call */
int   sora_rx11b_synchronize(sora_rx11b_t* rx);       /* every call issued so far has finished.  A handle keeps two calls in flight (own stream and result
                                                       * buffers each): process_dev waits only for the call before the previous one -- the caller's d_iq must
                                                       * stay untouched until then --, results reports the most recent call */
int  sora_rx11b_process_dev(sora_rx11b_t* rx, const sora_complex16* d_iq, const sora_capture_desc* caps, size_t ncaps);
int  sora_rx11b_process(sora_rx11b_t* rx, const sora_complex16* h_iq, size_t nsamples, const sora_capture_desc* caps, size_t ncaps);
int  sora_rx11b_results(sora_rx11b_t* rx, sora_frame_result* out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap);
/* Tickets, as for sora_rx_t: every process call has one; it stays valid until sora_rx11b_calls_in_flight() (2) further calls have reused its
 * slot (or, once the call is released -- delivered and waited for -- until the next call, which takes a released slot first) -- back-to-back calls are all collectable, each by its own
 * ticket, while the next one runs (what fb11b_demod.cpp does per frame,
 * per call).  The INPUT buffer of a call must stay untouched until sora_rx11b_wait(its ticket) (or _results_of, or _synchronize) has returned. */
int   sora_rx11b_ticket(sora_rx11b_t* rx);                     /* ticket of the most recent process call (0: none) */
int   sora_rx11b_calls_in_flight(sora_rx11b_t* rx);            /* how many calls the handle keeps addressable */
/* The graph runs as two kernels: the Barker-rate instantiation decodes every capture and hands those whose PLCP header announces 5.5 / 11 Mbps to the
 * CCK-capable one, which redoes them from their first sample.  enable = 1: every capture goes straight through the CCK-capable instantiation (all
 * four rates, identical rows) -- the better choice when most frames are CCK; 0: always two passes; 2 (DEFAULT since round 4): automatic -- a
 * two-pass call counts on the device how many captures its first pass handed over, and once such a count has come back (the handle never waits for
 * it) and says "more than half", the following calls take the single pass, except every 16th, which measures again; negative: query.  Returns the
 * previous setting (0, 1 or 2). */
int   sora_rx11b_set_single_pass(sora_rx11b_t* rx, int enable);
/* Which preambles the graph accepts.  mode 0 (DEFAULT): long only -- the reference's graph, whose TSFDSync knows one SFD; nothing changes, not a
 * row, not a byte.  mode 1: long and short -- the reference's graph with TSFDSync EXTENDED (the one place it moves; the front end locks well
 * inside the short SYNC and TDesc741 is self-synchronising, so nothing else in front changes).  THE RULE, per despread symbol, with a new state
 * bit_zero_found beside bit_one_found (both cleared by the graph's reset):
 *   - while neither is set: a window (the 16 most recent descrambled bits) of 0xFFFF sets bit_one_found, as in the reference; a window of
 *     0x0000 sets bit_zero_found once 16 symbols have gone in (the window starts out as zeros: until it is full, "all zeros" says nothing).
 *     The first to appear decides: the two are exclusive;
 *   - bit_one_found set: 0xF3A0 -> RATE_1M, any window other than 0xFFFF and 0xF3A0 counts towards bit_err_cnt (> 32: SFD_FAIL), as in the reference;
 *   - bit_zero_found set: 0x05CF -> the rate selector goes to RATE_2M with plcp_data still 0, so the six header bytes arrive through TDQPSKDemap
 *     (first reference symbol = the SFD's last, CF_DifferentialDemap::last_symbol) -> TDesc741 -> TBB11bPlcpSwitch -> TBB11bPlcpParser, which is
 *     untouched and sets the payload rate and length as ever; any window other than 0x0000 and 0x05CF counts towards bit_err_cnt, same > 32 rule;
 *   - the sync_cnt > 128 + 16 timeout (SFD_TIMEOUT) is unchanged.
 * Every row reported between a short SFD and the graph's next reset carries SORA_ROW_SHORT_PREAMBLE in flags; every other field means what it
 * means in mode 0.  Both pass plans and all settings of sora_rx11b_set_single_pass carry the mode.  Stream mode works with it unchanged: resume
 * points lie in plain carrier sense, where both flags are clear, so neither crosses a call.  Switching waits for the calls in flight (a call
 * runs wholly in one mode).  Negative: query.  Returns the previous mode. */
int   sora_rx11b_set_preamble(sora_rx11b_t* rx, int mode);
int   sora_rx11b_wait(sora_rx11b_t* rx, int ticket);
/* as sora_rx_wait_any: the oldest FINISHED call with an enqueued delivery; it is released and its slot reused first */
int   sora_rx11b_wait_any(sora_rx11b_t* rx, int* ticket);
void* sora_rx11b_stream_of(sora_rx11b_t* rx, int ticket);
int   sora_rx11b_results_of(sora_rx11b_t* rx, int ticket, sora_frame_result* out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap);
/* Result delivery without a host wait (as sora_rx_deliver_async): behind the call's kernels, on its stream, the dense rows in (capture, time)
 * order -- h_rows must have room for captures x max_frames_per_capture of them --, h_counts[0] = rows, h_counts[1] = MPDU bytes, and the MPDUs
 * densely packed in row order (the rows' mpdu_offset indexes h_mpdu; an MPDU that would reach past mpdu_cap is left out and h_counts[1] says
 * so).  mpdu_offset is the sum of the MPDU lengths (min(length, 4096) of the FRAME_OK / CRC32_FAIL rows) of all rows in front, whether or not those MPDUs
 * fitted and whether or not h_mpdu is given (unlike *_results_of, whose offsets count copied bytes); an MPDU is delivered exactly when mpdu_offset + its length
 * <= mpdu_cap, and h_counts[1] is the total, not what fitted.  A max_rows below captures x max_frames_per_capture is refused (SORA_ERR_CAPACITY) with nothing
 * enqueued.  Page-locked buffers (sora_hip_host_alloc); valid once sora_rx11b_wait(ticket) has returned.  h_mpdu may be NULL.
 * The copies are enqueued before the call's sizes are known to the host, so they move the WHOLE of what the caller offers -- max
 * captures x frames rows and all mpdu_cap bytes, every call: give mpdu_cap the size the traffic needs (frames x MTU), not a worst case
 * (rows x 4096 costs tens of MB over the host link per call and delivers stale bytes behind h_counts[1]). */
int   sora_rx11b_deliver_async(sora_rx11b_t* rx, int ticket, sora_frame_result* h_rows, size_t max_rows, uint32_t* h_counts, uint8_t* h_mpdu, size_t mpdu_cap);
/* Stream continuation, as sora_rx_set_stream_mode (the live-source case: a host binds CreateDemodGraph11b to TRxStream, and the graph's state --
 * the DC estimate, the energy detector, the facades a reset leaves alone, the harness's output buffer -- carries over from one read to the
 * next).  With sora_rx11b_set_stream_mode(rx, 1) capture k of a process call CONTINUES capture k of the call before it:
 *   - after a call, sora_rx11b_stream_consumed(rx, ticket, h, n) gives, per capture, the RESUME POINT: the number of 44 MHz samples of that
 *     capture that are final.  It is a source-call boundary in plain carrier sense (no frame under way, no event pending) with only whole
 *     28-sample calls in front of it; since the Seek behind a frame (352, 176, 64 or 32 samples) shifts the calls, it is a multiple of 4,
 *     not of 28 (0 if the capture holds none).  Every row the call reports ends at or in front of it (end_sample <= resume point); a frame
 *     still running at the end of the capture, or whose Seek the capture's end cut short, lies behind it and is NOT reported: the next call
 *     finds it again, so every frame is reported exactly once.  When a capture holds more row events than max_frames_per_capture, its resume
 *     point stops in front of the first event that found no row: no event is lost.  A zero-length capture leaves its stream as it was;
 *   - the host builds the next call's capture k from the stream FROM THAT POINT on: the unconsumed tail of what it submitted plus whatever
 *     has arrived since (capture lengths are still whole 28-sample source calls, offsets multiples of 4).  The library starts it with the
 *     state the graph had at the resume point, so the rows of all the calls together (positions relative to their own capture: add the
 *     stream position of its first sample) are exactly the events MAC11b_Receive reports on the uncut stream -- tests/test_gpu_stream11b.py
 *     holds streams cut at random source calls to the compiled reference graph's events on the whole;
 *   - calls of a handle in stream mode run one after the other (a process call first waits for both calls in flight: it needs their
 *     records); throughput comes from many streams (captures) per call.  Both process forms and every pass plan work in stream mode.
 *     sora_rx11b_stream_consumed exists for the most recent ticket only.  Switching the mode, either way, starts every stream afresh.
 * Returns the previous mode; a negative argument only queries. */
int   sora_rx11b_set_stream_mode(sora_rx11b_t* rx, int enable);
int   sora_rx11b_stream_consumed(sora_rx11b_t* rx, int ticket, uint32_t* h_consumed, size_t ncaps);

/* ------------------------------------------------------------------------------------------------
 * The bricks of the 802.11b receive graph as stage entry points: what CreateDemodGraph (fb11bdemod_config.hpp:122-172) is built from, each with the ports of the
 * brick it replaces, so that a host can replace ONE brick, or compose the graph from stages (sora_amd.rx11b_by_stages does):
 *     dc_remove -> energy_detect | symtiming -> barker_sync -> despread -> sfd_sync | dbpsk_demap / dqpsk_demap -> desc741 -> plcp_parse | frame_sink
 *                                                             cck5p5_decode / cck11_decode -> desc741 -> frame_sink
 * TBB11bRxSwitch, TBB11bRxRateSel and TBB11bPlcpSwitch only route and stay the host's.  The conventions are those of the stage entry points above: device
 * pointers, stream order, no allocation, no host wait; a null pointer gives SORA_ERR_INVALID_PARAM (sora_hip_last_error() names the function), no device
 * SORA_ERR_NO_DEVICE, nstreams = 0 is SORA_OK and launches nothing.  The bricks are stateful streams, so a call works on a BATCH of independent streams described by
 * device tables, as sora_hip_pilot_track11a does: stream f owns d_n[f] input units (a unit is the brick's burst: 4 samples, 11 chips, 8 symbols, ..) starting at
 * ELEMENT d_first[f] of d_in -- sample, chip, symbol or byte: a stream begins wherever the brick in front of it stopped swallowing -- and writes its output from element
 * d_out_first[f] of d_out.  What the brick keeps, and the context-facade fields it touches, lie in a per-stream
 * record, all 32-bit words, that the call reads and writes back: the state after the call is the state the brick would hold, and the same stream cut into two calls
 * gives what one call gives.  max_n bounds every d_n[f] (it sizes the grid; units of a stream at or behind it are not touched).  Offsets and buffers need no
 * alignment beyond their element's; the two record tables are 16- and 8-byte aligned.  Every stage equals tests/cxx/rx11b_stage_model.c bit for bit
 * (tests/test_gpu_11b_stages.py).  DESIGN.md section 7, f4b.
 * ------------------------------------------------------------------------------------------------ */
#define SORA_E_CS_TIMEOUT        ((int)0x80000007)  /* TEnergyDetect: 100 bursts without power (the harness resets the graph and does not report it) */
/* CF_11bRxMRSel::rxrate_state */
#define SORA_11B_RATE_SYNC 0
#define SORA_11B_RATE_1M   1
#define SORA_11B_RATE_2M   2
#define SORA_11B_RATE_5P5M 3
#define SORA_11B_RATE_11M  4
/* TBarkerSync::sync_flag */
#define SORA_11B_BARKER_SYNCED 4
/* what the demappers, the CCK decoders and TDesc741 carry: CF_DifferentialDemap::last_symbol, CF_Descramber::byte_reg (context: no Reset clears them) and
 * TCCK11Decoder's is_even (brick state, 0 after Reset).  Each stage reads and writes its own fields and leaves the others alone. */
typedef struct { sora_complex16 last_symbol; uint32_t byte_reg; uint32_t is_even; uint32_t reserved; } sora_stream11b_state;
/* TEnergyDetect + TDCEstimator; after Reset: all 0 but update_cnt = 8; cca_pwr_threshold and dc are context (the reference harness: 1000 * 1000; dc is never reset) */
typedef struct { uint32_t average_energy, window[8], idx, count, power_detected, error_code, cca_pwr_threshold, update_cnt; sora_complex16 sum_dc, dc; } sora_energy11b_state;
/* TSymTiming; after Reset: 2, 0 */
typedef struct { int32_t m_index, m_frag; } sora_symtiming11b_state;
/* TBarkerSync; after Reset: all 0 but last_peak_cnt = -1 */
typedef struct { int32_t sync_flag, last_peak_cnt, m_max, search_count; sora_complex16 partial[10]; uint32_t error_code; } sora_barker11b_state;
/* TSFDSync; after Reset: all 0 but last_symbol and byte_reg, which are context */
typedef struct { sora_complex16 last_symbol; uint32_t byte_reg, bit_one_found, bit_zero_found, word, bit_err_cnt, sync_cnt, rxrate_state, error_code; } sora_sfd11b_state;
typedef struct { uint32_t error_code, data_rate_kbps, frame_length, rxrate_state; } sora_plcp11b_rec;
typedef struct { uint32_t error_code, frame_crc32; } sora_sink11b_rec;

/* TDCRemove (Brick11/src/dc.hpp:6-38), 4 -> 4: out = wrap16(in - d_dc[f]); a unit is a burst of 4 samples */
int sora_hip_dc_remove11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, const sora_complex16* d_dc,
                          sora_complex16* d_out, size_t nstreams, size_t max_n, void* stream);
/* TEnergyDetect (cca.hpp:11-98) with the TDCEstimator (dc.hpp:92-166) it feeds, as one entry: stream f consumes bursts of 4 DC-removed samples until power_detected is set
 * or an error (SORA_E_CS_TIMEOUT) stands, d_n[f] at most; d_used[f] = the bursts consumed, the one that set power_detected included (it does not reach the estimator).
 * dc is reported as it stands afterwards; subtracting it is the host's TDCRemove.  A stream that enters with power_detected or error_code set consumes nothing. */
int sora_hip_energy_detect11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, sora_energy11b_state* d_state, uint32_t* d_used,
                              size_t nstreams, size_t max_n, void* stream);
/* TSymTiming (symtiming.hpp:10-170), 28 -> 1: d_n[f] blocks of 28 samples -> the decimated chips, 6, 7 or 8 per block, from chip d_out_first[f] of d_out (room for
 * 8 d_n[f]); d_nchips[f] = the chips written.  The state is a brick's: m_index in -1 .. 4. */
int sora_hip_symtiming11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_symtiming11b_state* d_state,
                          sora_complex16* d_out, uint32_t* d_nchips, size_t nstreams, size_t max_n, void* stream);
/* TBarkerSync (symtiming.hpp:176-315), 1 -> 1: swallows chips until the brick is BARKER_SYNCED; d_used[f] = the chips consumed before pass-through begins, or up to and
 * including the chip that raised SORA_E_SYNC_TIMEOUT (search_count >= 44).  The chips behind them are the brick's output and are not copied.  A stream that enters
 * synced or with error_code set consumes nothing. */
int sora_hip_barker_sync11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, sora_barker11b_state* d_state, uint32_t* d_used,
                            size_t nstreams, size_t max_n, void* stream);
/* TBB11bDespread (barkerspread.hpp:277-303), 11 -> 1: QuickBarkerDespread with its order of negate, >> 4 and wrapping sums.  Stateless. */
int sora_hip_despread11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_complex16* d_out,
                         size_t nstreams, size_t max_n, void* stream);
/* TSFDSync (sfd_sync.hpp:10-134), a sink of symbols: mode 0 is the reference's brick, mode 1 adds the short preamble by the rule stated at sora_rx11b_set_preamble.
 * Stream f consumes symbols up to and including the one that sets rxrate_state (RATE_1M, or RATE_2M behind a short SFD) or an error (SORA_E_SFD_FAIL,
 * SORA_E_SFD_TIMEOUT) -- one symbol can do both, and both are reported --; d_used[f] = the symbols consumed.  A stream that enters with either set consumes nothing. */
int sora_hip_sfd_sync11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, sora_sfd11b_state* d_state, uint32_t* d_used,
                         size_t nstreams, size_t max_n, int mode, void* stream);
/* TDBPSKDemap (barkerspread.hpp:312-390), 8 -> 1 byte, and TDQPSKDemap (:396-454), 4 -> 1 byte; state: last_symbol */
int sora_hip_dbpsk_demap11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_stream11b_state* d_state,
                            uint8_t* d_out, size_t nstreams, size_t max_n, void* stream);
int sora_hip_dqpsk_demap11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_stream11b_state* d_state,
                            uint8_t* d_out, size_t nstreams, size_t max_n, void* stream);
/* TCCK5P5Decoder (cck.hpp:70-206), 16 chips -> 1 byte; state: last_symbol.  TCCK11Decoder (cck.hpp:255-763), 8 chips -> 1 byte, the reference's pruned search (phi2 = 0
 * and pi/2, then the one of 3 pi/2 / pi that m1 > m2 picks) with its strict comparisons; state: last_symbol and is_even. */
int sora_hip_cck5p5_decode11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_stream11b_state* d_state,
                              uint8_t* d_out, size_t nstreams, size_t max_n, void* stream);
int sora_hip_cck11_decode11b(const sora_complex16* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_stream11b_state* d_state,
                             uint8_t* d_out, size_t nstreams, size_t max_n, void* stream);
/* TDesc741 (scramble.hpp:93-170), 1 -> 1 byte: z^-7 + z^-4 + 1, self-synchronising; state: byte_reg */
int sora_hip_desc741_11b(const uint8_t* d_in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, sora_stream11b_state* d_state,
                         uint8_t* d_out, size_t nstreams, size_t max_n, void* stream);
/* TBB11bPlcpParser (PHY_11b.hpp:524-640): d_hdr[f][6] -> d_rec[f] (16-byte aligned): error_code 0 or SORA_E_PLCP_HEADER_FAIL (the CRC-16; the other fields are then 0),
 * data_rate_kbps (0 for an unknown SIGNAL, with frame_length 0 and rxrate_state 0 = "unchanged"), frame_length by the four length formulas with the SERVICE bits,
 * rxrate_state (SORA_11B_RATE_*) */
int sora_hip_plcp_parse11b(const uint8_t* d_hdr, sora_plcp11b_rec* d_rec, size_t nstreams, void* stream);
/* TBB11bFrameSink (PHY_11b.hpp:643-749) over one frame per stream: the descrambled bytes of frame f from byte d_first[f] of d_bytes, d_len[f] = frame_length (<= 65535).
 * d_rec[f] (8-byte aligned) = error_code SORA_E_FRAME_OK / SORA_E_CRC32_FAIL (0 where the brick raises nothing: lengths below 4) and frame_crc32 = the three FCS bytes the
 * sink holds when it decides, the fourth byte 0 (the brick: a stale buffer byte).  The sink decides one byte early: byte frame_length - 1 is never read.  Bytes from index
 * 4096 on lie behind the brick's buffer: they count for the CRC and read back as 0. */
int sora_hip_frame_sink11b(const uint8_t* d_bytes, const uint32_t* d_first, const uint32_t* d_len, sora_sink11b_rec* d_rec, size_t nstreams, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Small device-memory helpers so a pure-C host needs no HIP headers.
 * ------------------------------------------------------------------------------------------------ */
int   sora_hip_device_count(void);

/* The look-up tables (usin / ucos / uatan2 of core/inc/intalglut.h:4,3648,7332, the FFT twiddles of fft_lut_twiddle.h:61433-61600, the demapper's step tables of
 * Brick11/src/demapper.h:55-130, dsp_math.h:215-245's sincos / atan, ...) are regenerated from closed forms when a process first needs them, with the host's libm.
 * Each has a PINNED sha256 compiled into the library; a table that does not hash to its pin (another libm, -ffast-math) makes every create / stage call fail with
 * SORA_ERR_FAILED instead of decoding differently.  sora_hip_table_digest needs no device; sora_hip_table_read copies the device-resident table of the current
 * device back (h_out == NULL: only *bytes). */
int   sora_hip_table_count(void);
const char* sora_hip_table_name(int index);
const char* sora_hip_table_pin(const char* name);                 /* the pinned sha256 (64 hex digits), NULL: no such table */
int   sora_hip_table_digest(const char* name, char hex65[65]);    /* what this build on this host generates */
int   sora_hip_table_read(const char* name, void* h_out, size_t cap, size_t* bytes);
void* sora_hip_malloc(size_t bytes);
void  sora_hip_free(void* d_ptr);
int   sora_hip_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int   sora_hip_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
int   sora_hip_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes, void* stream);   /* asynchronous on `stream` */
/* page-locked host memory (the target of asynchronous result delivery) */
void* sora_hip_host_alloc(size_t bytes);
void  sora_hip_host_free(void* h_ptr);
/* wait for a stream (NULL = the null stream); the streams of a sora_rx_t do not follow the null stream */
int   sora_hip_stream_synchronize(void* stream);
int   sora_hip_abi_version(void);
const char* sora_hip_last_error(void);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SORA_HIP_H */
