// kernels.h -- argument blocks and declarations of the receive-path kernels (shared by host and device code).
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "dev_arith.h"
#include "rx_types.h"
#include "../../include/sora_hip.h"

// Probe switches (SORA_SCAN_PROBE, SORA_DBG_*) belong to the TOOLS variant of the library (sora_amd.build.build_variant adds -DSORA_TOOLS for them): the product
// build refuses them, so no measurement scaffolding can reach it by accident.
#if !defined(SORA_TOOLS) && (defined(SORA_SCAN_PROBE) || defined(SORA_DBG_PIPE_TIMELINE) || defined(SORA_DBG_PIPE_LOSE_FLAGS) || defined(SORA_DBG_SYMT_NO_SCAN))
#error "SORA_SCAN_PROBE / SORA_DBG_* switches need -DSORA_TOOLS (sora_amd.build.build_variant)"
#endif

namespace sora {

struct ScanArgs {
    const uint32_t* iq;         // packed COMPLEX16
    const CapDesc*  caps;
    uint32_t        ncaps;
    uint32_t        str;        // 2: 40 MHz input (keep even samples), 1: 20 MHz input
    uint32_t        keep_queue; // 1: the 44 MHz graph (TDownSample44_40 has no Reset/Flush: its queued samples survive a frame reset)
    uint32_t        thr;        // cca_pwr_threshold
    uint32_t        max_frames; // per capture
    Tables          T;
    FrameRow*       frames;     // [ncaps*max_frames]
    FrameCtx*       fctx;
    uint32_t*       nframes;    // [ncaps]
    uint32_t*       njobs;      // [3] frames whose data symbols must be decoded, per code rate (1/2, 2/3, 3/4)
    uint32_t*       joblist;    // [3][nrows] their frame-table rows, compacted: consecutive workgroups of the per-frame
                                //            kernels then carry live work (workgroup b runs on XCD b % 8)
    uint32_t        nrows;      // list stride = ncaps * max_frames
    uint32_t*       slot_row;   // [total slots] frame-table row that owns a symbol slot (the data symbols of every queued frame); the host presets 0xFFFFFFFF
    // stream continuation (sora_rx_set_stream_mode): capture k of this call continues capture k of the call before it
    // [ncaps][kContWords] the carrier-sense state at the capture's last resume point (read at entry when valid, rewritten at every later one); null = off
    uint32_t*       cont;
    uint32_t*       consumed;   // [ncaps] input-rate samples of this capture that are final: the host submits the stream from there on next time
    // what the NEXT call needs cleared, done here instead of by a fill kernel in front of every call (sora_hip.cpp: a pipeline's calls alternate between two sets of
    // job counters; workgroup 0 zeroes the set this call does not use, and k_pipe's hand-off words): null = the host's fill has done it
    uint32_t*       zero_a; uint32_t nzero_a;
    uint32_t*       zero_b; uint32_t nzero_b;
    uint32_t        own_slots;  // 1: every capture's workgroup presets its own symbol slots' owners (0xFFFFFFFF) itself
};
constexpr int kContWords = 64;

struct RxArgs {
    const uint32_t* iq;
    const CapDesc*  caps;
    uint32_t        str;
    uint32_t        total_slots;
    uint32_t        nrows;          // ncaps*max_frames
    Tables          T;
    FrameRow*       frames;
    const FrameCtx* fctx;
    uint8_t*        soft;           // [slots*288 + pad] the frames' soft streams (one byte per value, v << 1: rx_types.h)
    uint8_t*        vout;           // [slots*32]
    uint8_t*        mpdu;           // [slots*32]
    VitJob*         jobs;           // [3][nrows] (indexed by job)
    const uint32_t* njobs;
    const uint32_t* joblist;
    const uint32_t* slot_row;       // [total_slots] owner row of a symbol slot, 0xFFFFFFFF = none (k_scan)
    uint32_t*       eq;             // [total_slots][64] equalised bins, packed COMPLEX16 (k_sym_front -> k_track_lds, k_sym_back)
    TrackRec*       track;          // [total_slots] rotation parameters of a data symbol (k_track_lds -> k_sym_back)
    uint32_t*       pil;            // [total_slots][4] the four pilot bins (43, 57, 7, 21) of eq[] once more, densely: all k_track_lds reads
    const uint32_t* pipe_flags;     // k_finish behind k_pipe: word 0 != 0 = a hand-off inside that launch gave up (else null)
    // sora_rx_bind_mpdu: the caller's page-locked MPDU array (the geometry of mpdu[]): the frame sink writes every MPDU there as well, over PCIe, as it finishes the frame (else null)
    uint8_t*        mpdu_host;
};

// k_pipe (k_rx.hip): the data field of a handful of frames as ONE launch.  Workgroups [0, nfront) are k_sym_front's, [nfront, nfront + ntrack) one frame's tracker and
// everything behind it each, the rest four waves of the window-parallel trellis.  flags (zeroed before every call): [0] a wait gave up; [4 + 4 f + h] quads of symbols
// published by helper wave h of frame row f; [4 + 4 nrows + b] front workgroup b is done.
struct PipeArgs {
    uint32_t  nfront, ntrack;
    uint32_t* flags;
    uint32_t  target, vstride;     // the window-parallel trellis's unit target and its vectors' stride per code-rate list
    uint16_t* vecs;
    uint32_t  stamp_base;          // (tools variant, SORA_DBG_PIPE_TIMELINE: where the launch's time stamps go, in words from flags)
    uint32_t  lanes64;             // 1: the trellis role decodes its units two per wave in the 64-lane layout (a lone capture: a third faster per unit), 0: eight per wave
    uint32_t  wait_ticks;          // bound of every wait inside the launch, in ticks of the 100 MHz counter (sora_rx_set_pipe_wait_us)
};

__global__ void k_scan(ScanArgs A);
__global__ void k_frame(RxArgs A);
__global__ void k_sym_front(RxArgs A);
__global__ void k_track_lds(RxArgs A);
__global__ void k_sym_back(RxArgs A);
__global__ void k_pipe(RxArgs A, PipeArgs P);
__global__ void k_viterbi(const VitJob* jobs, const uint32_t* njobs3, uint32_t njobs_single, uint32_t stride, const uint8_t* soft, uint8_t* out);
__global__ void k_viterbi_p3(const VitJob* jobs, const uint32_t* njobs3, uint32_t njobs_single, uint32_t stride, const uint8_t* soft, uint8_t* out);
__global__ void k_viterbi11n(const VitJob* jobs, const uint32_t* njobs3, uint32_t njobs_single, uint32_t stride, const uint8_t* soft, uint8_t* out);
// k_vit56.hip: code rate 5/6, a job table's fourth list (njobs[3] jobs at jobs + 3 stride); span = bytes of the soft buffer: nothing at or behind it is read
__global__ void k_viterbi56_11n(const VitJob* jobs, const uint32_t* njobs, uint32_t stride, const uint8_t* soft, uint32_t span, uint8_t* out);
// k_vit16.hip
__global__ void k_viterbi16(const VitJob* jobs, const uint32_t* njobs3, uint32_t njobs_single, uint32_t stride, const uint8_t* soft, uint8_t* out);
__global__ void k_viterbi16_p3(const VitJob* jobs, const uint32_t* njobs3, uint32_t njobs_single, uint32_t stride, const uint8_t* soft, uint8_t* out);
__global__ void k_viterbi16_11n(const VitJob* jobs, const uint32_t* njobs3, uint32_t njobs_single, uint32_t stride, const uint8_t* soft, uint8_t* out);
// k_vitwin.hip: the window-parallel trellis.  hdr = the call's counter block (njobs per code rate in its first three words); jstride = capacity of a list of jobs;
// target = units the call is cut into at least, frames permitting; vstride = vectors per code-rate list
__global__ void k_viterbi16w(const VitJob* jobs, const uint32_t* hdr, uint32_t jstride, uint32_t target, uint32_t vstride, const uint8_t* soft, uint8_t* out, uint16_t* vecs);
__global__ void k_viterbi16w_p3(const VitJob* jobs, const uint32_t* hdr, uint32_t jstride, uint32_t target, uint32_t vstride, const uint8_t* soft, uint8_t* out, uint16_t* vecs);
__global__ void k_viterbi16w_11n(const VitJob* jobs, const uint32_t* hdr, uint32_t jstride, uint32_t target, uint32_t vstride, const uint8_t* soft, uint8_t* out, uint16_t* vecs);
__global__ void k_win_redo_11n(const VitJob* jobs, const uint32_t* hdr, uint32_t jstride, uint32_t target, uint32_t vstride, const uint16_t* vecs,
        const uint8_t* soft, uint8_t* out, unsigned long long* stats);
__global__ void k_win_redo(const VitJob* jobs, const uint32_t* hdr, uint32_t jstride, uint32_t target, uint32_t vstride, const uint16_t* vecs,
        const uint8_t* soft, uint8_t* out, unsigned long long* stats);
__global__ void k_win_redo_p3(const VitJob* jobs, const uint32_t* hdr, uint32_t jstride, uint32_t target, uint32_t vstride, const uint16_t* vecs,
        const uint8_t* soft, uint8_t* out, unsigned long long* stats);
__global__ void k_win_redo_finish(const VitJob* jobs, const uint32_t* hdr, uint32_t jstride, uint32_t target, uint32_t vstride, const uint16_t* vecs,
        const uint8_t* soft, uint8_t* out, unsigned long long* stats,
                                  RxArgs A);   // ... and k_finish behind it, in the same waves   // k_rx.hip
// ... behind k_pipe: the same, and the plain chain's code for the whole call if a hand-off inside k_pipe gave up (host_note: a host-mapped word that is set then)
__global__ void k_win_redo_finish_pipe(const VitJob* jobs, const uint32_t* hdr, uint32_t jstride, uint32_t target, uint32_t vstride, const uint16_t* vecs,
        const uint8_t* soft, uint8_t* out, unsigned long long* stats, RxArgs A, uint32_t* host_note);
__global__ void k_finish(RxArgs A);
struct PackedRow;
__global__ void k_pack(const FrameRow* frames, const uint32_t* nframes, const CapDesc* caps, uint32_t ncaps, uint32_t max_frames, PackedRow* rows, uint32_t* nrows_out);
struct TxArgs {                // sora_hip_tx11a (k_tx.hip)
    const uint8_t*  mpdu;      // MPDUs without FCS, frame f at mpdu + off[f]
    const uint32_t* off;
    const uint32_t* len;       // bytes without FCS (LENGTH = len + 4)
    const uint32_t* rate;      // kbps
    const uint8_t*  seed;      // scrambler register before the first byte (the harness uses 0xFF)
    int8_t*         out8;      // COMPLEX8 stream
    const uint64_t* out_off;   // first sample of frame f
    const int8_t*   preamble;  // 640 samples (UP44: 704)
    Tables          T;
};
__global__ void k_tx_preamble(int8_t* out8, int8_t* out44, Tables T);   // 640 samples at 40 MHz, 704 at 44 MHz
template <bool UP44> __global__ void k_tx11a(TxArgs A);                 // UP44: TUpsample40MTo44M in front of the 16 -> 8 bit pack (sora_hip_tx11a44)

// ---- 802.11n 2x2 transmitter (k_tx11n.hip)
struct Tx11nArgs {             // sora_hip_tx11n
    const uint8_t*  mpdu;      // MPDUs without FCS, frame f at mpdu + off[f]
    const uint32_t* off;
    const uint32_t* len;       // bytes without FCS (HT LENGTH = len + 4)
    const uint32_t* mcs;       // 8..14
    const uint8_t*  seed;      // scrambler register before the first byte; nullptr: 0xAB for every frame (fb11nmod_config.hpp:51)
    uint32_t*       out0;      // packed COMPLEX16, TX chain 0
    uint32_t*       out1;      // TX chain 1
    const uint64_t* out_off;   // first sample of frame f in both streams
    const uint32_t* preamble;  // [2][1120]: per chain L-STF, L-LTF (640) then HT-STF, HT-LTF1, HT-LTF2 (480)
    Tables          T;
};
// MCS 8..14 of both HT transmitters (DOT11N_RATE_PARAMS, BB11nGetCodingRateFromMcsIndex): N_BPSC, the code rate R (cr: 0 = 1/2, 1 = 2/3, 2 = 3/4) and
// dbpc2 = 2 N_BPSC R -- twice the data bits one carrier of one stream holds (1/2, 1, 3/2, 2, 3, 4, 9/2 for MCS 8..14), so that a plan's N_DBPS is one
// multiplication: (data carriers per symbol, all streams) / 2 x dbpc2.  The plans run on the device too: no division by a run-time rate.
__host__ __device__ inline bool tx_ht_mcs(uint32_t mcs, int& nb, int& cr, int& dbpc2)
{
    switch (mcs) {
    case 8:  nb = 1; cr = 0; dbpc2 = 1; break;  case 9:  nb = 2; cr = 0; dbpc2 = 2; break;
    case 10: nb = 2; cr = 2; dbpc2 = 3; break;  case 11: nb = 4; cr = 0; dbpc2 = 4; break;
    case 12: nb = 4; cr = 2; dbpc2 = 6; break;  case 13: nb = 6; cr = 1; dbpc2 = 8; break;
    case 14: nb = 6; cr = 2; dbpc2 = 9; break;
    default: return false;
    }
    return true;
}
// The frame geometry the reference's data graph produces (PHY_11n.hpp:15-150, ieee80211n_cmn.h:34-55, pinqueue.h:133-147).
// TBB11nSrc emits nbytes = ceil(nstd * NDBPS / 8) bytes (nstd: the standard's symbol count); on Flush every pipe pads its
// last burst with zeros -- the encoder's input to a whole group (1, 2 or 3 bytes for rate 1/2, 2/3, 3/4), the stream parser's
// input to a whole symbol -- so the field carries nvalid input bits and nsym = ceil(coded bytes / 13 N_BPSC) symbols, one more
// than nstd whenever nstd * NDBPS is not a multiple of 8 (MCS 8, 10 and 14 with odd nstd).
struct Tx11nPlan { int nb, cr, ndbps; uint32_t nstd, nbytes, nvalid, nsym; };
__host__ __device__ inline bool tx11n_plan(uint32_t len, uint32_t mcs, Tx11nPlan& P)
{
    if (len < 1 || len > 4092) return false;
    int dbpc2;
    if (!tx_ht_mcs(mcs, P.nb, P.cr, dbpc2)) return false;   // MCS 15 goes to TDropAny: no frame
    P.ndbps = 52 * dbpc2;                                // two streams of 52 data carriers
    const uint32_t nd = (uint32_t)P.ndbps, gin = (uint32_t)P.cr + 1, gout = (uint32_t)P.cr + 2;
    P.nstd = ((len + 4) * 8 + 16 + 6 + nd - 1) / nd;     // SERVICE 16 bits, tail 6 bits
    P.nbytes = (P.nstd * nd + 7) / 8;
    const uint32_t ngroups = (P.nbytes + gin - 1) / gin;
    P.nvalid = 8 * gin * ngroups;
    P.nsym = (gout * ngroups + 13 * (uint32_t)P.nb - 1) / (13 * (uint32_t)P.nb);
    return true;
}
constexpr uint32_t kTx11nPreamble = 1120;                // samples per chain of the table: L-STF + L-LTF + HT-STF + 2 HT-LTF
__global__ void k_tx11n(Tx11nArgs A);

// k_mod11n.hip: LSrc / HTSrc as a stage, launched beside the transmitter whose table it copies (sora_hip_preamble11n); nwords 16-byte words
__global__ void k_mod11n_preamble(const uint4* table, uint4* out0, uint4* out1, uint32_t w0, uint32_t nw, uint64_t nwords);

// ---- 40 MHz HT 2x2 transmitter (k_tx_ht40.hip)
struct TxHt40Args {            // sora_hip_tx_ht40; sora_hip_tx_ht40_joint: ONE MPDU and one seed per frame -- off[nframes], seed[nframes] (nullptr: 0x5D)
    const uint8_t*  mpdu;      // MPDUs without FCS: stream s of frame f at mpdu + off[2 f + s]
    const uint32_t* off;       // [2 nframes]
    const uint32_t* len;       // [nframes] bytes without FCS, the same for both streams (HT LENGTH = len + 4)
    const uint32_t* mcs;       // 8..14
    const uint8_t*  seed;      // [2 nframes] scrambler seeds (py_ht40.scramble_seq's, 7 bits used); nullptr: 0x5D, 0x2B
    uint32_t*       out0;      // packed COMPLEX16, TX chain 0 (spatial stream 0)
    uint32_t*       out1;      // TX chain 1
    const uint64_t* out_off;   // first sample of frame f in both streams
    const uint32_t* preamble;  // [2][1120]: per chain L-STF, L-LTF (640) then HT-STF, HT-LTF1, HT-LTF2 (480), k_tx_ht40_preamble
    Tables          T;
    const uint8_t*  gi;        // per frame: 0 = long guard interval, 1 = short; nullptr: all long.  Read by k_tx_ht40_gi / k_tx_ht40_joint_gi only (sora_hip_tx_ht40_gi)
};
// N_SYM = ceil((16 + 8 (len + 4) + 6) / N_DBPS) with N_DBPS = 108 N_BPSC R: sora_ht40_symbols(len + 4, len + 4, nb, cr), py_ht40.nsym_for
struct TxHt40Plan { int nb, cr, ndbps; uint32_t nsym; };
__host__ __device__ inline bool tx_ht40_plan(uint32_t len, uint32_t mcs, TxHt40Plan& P)
{
    if (len < 1 || len > 3996) return false;             // HT LENGTH <= 4000, the receiver's limit
    int dbpc2;
    if (!tx_ht_mcs(mcs, P.nb, P.cr, dbpc2)) return false;
    P.ndbps = 54 * dbpc2;                                // 108 data carriers per stream
    P.nsym = (16u + 8u * (len + 4u) + 6u + (uint32_t)P.ndbps - 1u) / (uint32_t)P.ndbps;
    return true;
}
// The joint coding (sora_hip_tx_ht40_joint): ONE PSDU through one scrambler and one encoder, stream-parsed over the two streams, so a
// symbol carries N_DBPS = 2 x 108 N_BPSC R data bits: N_SYM = sora_ht40_symbols_joint(len + 4, nb, cr)
__host__ __device__ inline uint32_t ht40_symbols_joint(uint32_t length, uint32_t ndbps_joint) { return (16u + 8u * length + 6u + ndbps_joint - 1u) / ndbps_joint; }
__host__ __device__ inline bool tx_ht40_plan_joint(uint32_t len, uint32_t mcs, TxHt40Plan& P)
{
    if (len < 1 || len > 3996) return false;             // HT LENGTH <= 4000, the receiver's limit
    int dbpc2;
    if (!tx_ht_mcs(mcs, P.nb, P.cr, dbpc2)) return false;
    P.ndbps = 108 * dbpc2;                               // 108 data carriers on each of the two streams
    P.nsym = ht40_symbols_joint(len + 4u, (uint32_t)P.ndbps);
    return true;
}
// MCS 15: the two plans behind a gate.  mcs_max 14: the plans above, whatever the MCS; 15: MCS 15 is accepted too -- 64-QAM, rate 5/6
// (SORA_CR_56 = 3), N_DBPS = 540 per stream, 1080 over both in the joint coding; any other gate accepts nothing.
__host__ __device__ inline bool tx_ht40_plan_mcs(uint32_t len, uint32_t mcs, uint32_t mcs_max, bool joint, TxHt40Plan& P)
{
    if (mcs_max != 14 && mcs_max != 15) return false;
    if (mcs != 15 || mcs_max != 15) return joint ? tx_ht40_plan_joint(len, mcs, P) : tx_ht40_plan(len, mcs, P);
    if (len < 1 || len > 3996) return false;
    P.nb = 6; P.cr = 3; P.ndbps = joint ? 1080 : 540;
    P.nsym = (16u + 8u * (len + 4u) + 6u + (uint32_t)P.ndbps - 1u) / (uint32_t)P.ndbps;
    return true;
}
constexpr uint32_t kTxHt40Preamble = 1120;               // samples per chain of the table: L-STF + L-LTF + HT-STF + 2 HT-LTF
constexpr int kTxHt40Amp = 16384;                        // A: the bin value of an LTF / SIG carrier (tests/tx_ht40_model.py)
__global__ void k_tx_ht40_preamble(uint32_t* tab, Tables T);
__global__ void k_tx_ht40(TxHt40Args A);
__global__ void k_tx_ht40_joint(TxHt40Args A);
// The short guard interval: a frame's kind (TxHt40Args::gi) selects the data symbols' pitch and emission, HT-SIG bit 31 and the L-SIG length.
// Samples per chain: the fields up to HT-LTF 2 keep their 160-sample symbols; a short data symbol is the last 16 of its 128 samples, then the 128.
constexpr uint32_t kHt40ShortSym = 144, kHt40ShortCp = 16;
// raw captures: how much later than a20 says a short-GI frame's data field is taken (k_ht40_plan), and what a stream piece must hold behind the frame's extent for that
constexpr uint32_t kHt40ShortAdvance = 16;
__host__ __device__ inline size_t tx_ht40_frame_samples(uint32_t nsym, uint32_t gi) { return 1600u + (size_t)(gi ? kHt40ShortSym : 160u) * nsym; }
// L-SIG LENGTH = 3 x (the 4 us symbols behind L-SIG, rounded up) - 3: 3 + nsym data symbols of 4 us, or of 3.6 us rounded up to whole 4 us
__host__ __device__ inline uint32_t tx_ht40_lsig_length(uint32_t nsym, uint32_t gi) { return 12u + 3u * (gi ? (9u * nsym + 9u) / 10u : nsym); }
__global__ void k_tx_ht40_gi(TxHt40Args A);
__global__ void k_tx_ht40_joint_gi(TxHt40Args A);
// ... and with the gate at 15 (sora_hip_tx_ht40_mcs, sora_hip_tx_ht40_joint_mcs): the guard-aware kernels that also accept MCS 15
__global__ void k_tx_ht40_mcs(TxHt40Args A);
__global__ void k_tx_ht40_joint_mcs(TxHt40Args A);
// k_mod_ht40.hip: the fixed fields as a stage, launched beside the transmitter whose table it copies (sora_hip_preamble_ht40); nwords 16-byte words
__global__ void k_mod_ht40_preamble(const uint4* table, uint4* out0, uint4* out1, uint32_t w0, uint32_t nw, uint64_t nwords);

// ---- 802.11b transmitter (k_tx11b.hip)
struct Tx11bArgs {             // sora_hip_tx11b
    const uint8_t*  mpdu;      // MPDUs without FCS, frame f at mpdu + off[f]
    const uint32_t* off;
    const uint32_t* len;       // bytes without FCS
    const uint32_t* rate;      // kbps: 1000, 2000, 5500, 11000
    const uint8_t*  phase_in;  // CF_DifferentialMap::last_phase before the frame (0..3); nullptr: 0
    uint8_t*        phase_out; // last_phase after the frame; nullptr: not written
    int8_t*         out;       // COMPLEX8 at 44 MHz
    const uint64_t* out_off;   // first sample of frame f
    Tables          T;
    const uint8_t*  preamble;  // per frame: 0 = long, 1 = short; nullptr: all long (sora_hip_tx11b_pre)
};
// The PPDU is a header (SYNC, SFD, PLCP header) spread over Barker, then MPDU + FCS at the frame's rate: cpb chips a byte in symbols of
// ls chips, spb symbols a byte.  The header's geometry is stated here once, for the host's sample count and for the kernel:
//   preamble 0 (long):  16 x 0xFF, SFD 0xF3A0, six PLCP bytes, all 24 at 1 Mbps DBPSK (88 chips a byte); scrambler register 0x6C
//   preamble 1 (short):  7 x 0x00, SFD 0x05CF at 1 Mbps DBPSK (9 bytes), the six PLCP bytes at 2 Mbps DQPSK (44 chips a byte);
//                        scrambler register 0x1B; payload at 2, 5.5 or 11 Mbps only (kernel/inc/dot11_plcp.h's short-preamble constants)
// hb1 bytes of the header go out as DBPSK, hb - hb1 as DQPSK: hsyms symbols of 11 chips, hchips chips.  TQuickPulseShaper emits four
// samples per chip and five more chip steps at Flush; the last burst of eight samples is padded: the sample count is 4 nchips + 24.
struct Tx11bPlan { uint32_t code, cpb, ls, spb, nchips, hb1, hb, hsyms, hchips, sync, sfd, seed; };
__host__ __device__ inline bool tx11b_plan(uint32_t len, uint32_t rate_kbps, Tx11bPlan& P, uint32_t preamble = 0)
{
    if (len < 1 || len > 4092 || preamble > 1) return false;
    switch (rate_kbps) {                                   // SIGNAL: the rate in units of 100 kbit/s
    case 1000:  P.code = 0x0A; P.cpb = 88; P.ls = 11; P.spb = 8; break;   // DBPSK, Barker
    case 2000:  P.code = 0x14; P.cpb = 44; P.ls = 11; P.spb = 4; break;   // DQPSK, Barker
    case 5500:  P.code = 0x37; P.cpb = 16; P.ls = 8;  P.spb = 2; break;   // CCK, 4 bits a symbol
    case 11000: P.code = 0x6E; P.cpb = 8;  P.ls = 8;  P.spb = 1; break;   // CCK, 8 bits a symbol
    default: return false;
    }
    if (preamble == 0) { P.hb1 = 24; P.hb = 24; P.sync = 0xFF; P.sfd = 0xF3A0; P.seed = 0x6C; }   // DOT11B_PLCP_LONG_*
    else {
        if (rate_kbps == 1000) return false;               // (no 1 Mbps frame behind a short preamble)
        P.hb1 = 9; P.hb = 15; P.sync = 0x00; P.sfd = 0x05CF; P.seed = 0x1B;                          // DOT11B_PLCP_SHORT_*
    }
    P.hsyms = 8 * P.hb1 + 4 * (P.hb - P.hb1);
    P.hchips = 11 * P.hsyms;
    P.nchips = P.hchips + (len + 4) * P.cpb;
    return true;
}
__global__ void k_tx11b(Tx11bArgs A);

// the 802.11b modulation graph's bricks as stages (k_mod11b.hip): a workgroup per stream, in passes of kMod11bT input units (bytes; chips for the shaper)
constexpr int kMod11bT = 1024;
__global__ void k_ingest(const uint8_t* raw, uint32_t* out, uint64_t m0, uint64_t n_out, unsigned flags);
__global__ void k_ingest_tile(const uint8_t* raw, uint32_t* out, unsigned flags, uint32_t tiles);
__global__ void k_soft_pack3(const uint8_t* soft8, const uint32_t* off8, const uint32_t* nsoft, const uint16_t* flen, const uint32_t* out_off,
                             int code_rate, uint8_t* packed, VitJob* jobs);
__global__ void k_soft_jobs8(const uint32_t* off8, const uint32_t* nsoft, const uint16_t* flen, const uint32_t* out_off, int code_rate, uint32_t n, VitJob* jobs);

// ---- 802.11b receive graph (k_rx11b.hip)
struct Rx11bRow { uint32_t end_sample, error_code, rate_kbps, length, crc32; };
// 802.11b rows only: rate_kbps bit 31 = the frame came behind the short preamble; delivery (k_deliver.hip) moves it to SORA_ROW_SHORT_PREAMBLE
constexpr uint32_t kRowShortBit = 0x80000000u;
struct Rx11bArgs {
    const uint32_t* iq;         // packed COMPLEX16 @44 MHz
    const CapDesc*  caps;
    uint32_t        ncaps;
    uint32_t        thr;        // cca_pwr_threshold
    uint32_t        max_frames; // rows per capture
    Rx11bRow*       rows;       // [ncaps*max_frames]
    uint32_t*       nframes;    // [ncaps]
    uint8_t*        mpdu;       // [ncaps*max_frames][4096]
    const uint32_t* crc;        // CRC-32 table
    // [ncaps]: set by the first pass for a capture in which a header announces 5.5 / 11 Mbps; such captures are redone by k_rx11b_cck
    uint32_t*       needs_cck;
    // stream continuation (sora_rx11b_set_stream_mode): capture k of this call continues capture k of the call before it; null = off
    uint32_t*       cont;       // [ncaps][kRec11bWords] the continuation records: read at entry, rewritten by the pass that finishes the capture
    uint32_t*       consumed;   // [ncaps] the capture's last resume point, in 44 MHz samples: the host submits the stream from there on next time
};
constexpr uint32_t kRec11bWords = 64 + 2 * 1024;    // registers and energy window, then two copies of the 4 KiB output buffer (k_rx11b.hip)
__global__ void k_rx11b(Rx11bArgs A);
__global__ void k_rx11b_cck(Rx11bArgs A);
__global__ void k_rx11b_stream(Rx11bArgs A);        // the same two passes, in stream form
__global__ void k_rx11b_cck_stream(Rx11bArgs A);
__global__ void k_rx11b_pre(Rx11bArgs A);           // the same four with TSFDSync extended to the short preamble (sora_rx11b_set_preamble)
__global__ void k_rx11b_cck_pre(Rx11bArgs A);
__global__ void k_rx11b_stream_pre(Rx11bArgs A);
__global__ void k_rx11b_cck_stream_pre(Rx11bArgs A);

// a continuation record of the 802.11n / HT40 front ends' stream forms (k_rx11n.hip): header, the four MimoAutoCorr rings of both chains, the 64 delayed energies
constexpr uint32_t kRec11nWords = 64 + 4 * 64 + 128;
// one event of the 40 MHz HT front end (k_scan_ht40 in k_rx11n.hip), row cap * max_frames + i
struct Ht40Found {
    uint32_t a20;                  // 20 MHz index (in the capture) of the first HT-STF sample: HT-LTF 1 starts 2 * a20 + 160 samples @40 MHz into the capture
    uint32_t mcs, ht_len, nsym;    // 0 unless the frame was recorded
    int32_t  cfo;                  // phase step per 20 MHz sample, 65536 = 2 pi (TFreqOffsetEst_11n's convention)
    float    noise_var;            // per carrier of the FFT<128> of the 40 MHz stream, LSB^2 (from the L-LTF pair)
    uint32_t end_sample;           // 40 MHz source position at which the event is seen
    uint32_t error_code;           // 0: recorded (the data field decides), else E_PLCP
};

}  // namespace sora

// d_cont / d_consumed: the streams' continuation records [ncaps][kRec11nWords] and resume points [ncaps] (k_scan_ht40_stream); null = k_scan_ht40
// joint: 1 = a frame's extent follows the joint coding's N_SYM (sora_ht40_set_coding)
// guard: 1 = SORA_HT40_GUARD_SIGNALLED (sora_ht40_set_guard): k_scan_ht40_gi / k_scan_ht40_stream_gi, which read HT-SIG's Short GI bit
int sora_internal_scan_ht40(const uint32_t* iq0, const uint32_t* iq1, const sora::CapDesc* d_caps, uint32_t ncaps, uint32_t max_frames, sora::Rx11bRow* d_rows, uint32_t* d_nframes,
                            sora::Ht40Found* d_found, const sora::Tables& T, const uint32_t* sincos, const short* atan, hipStream_t st,
                            uint32_t* d_cont = nullptr, uint32_t* d_consumed = nullptr, uint32_t joint = 0, uint32_t guard = 0, uint32_t mcs_max = 14);

// k_deliver.hip: dense rows + MPDUs of a call of the Rx11bRow-table handles into page-locked host memory, behind the call's kernels
struct DenseStage {                  // per slot / pipeline (grow-only device staging)
    sora_frame_result* d_rows = nullptr; size_t rows_bytes = 0;
    uint32_t* d_src = nullptr; size_t src_bytes = 0;
    uint8_t* d_mpdu = nullptr; size_t mpdu_bytes = 0;
    uint32_t* d_meta = nullptr; size_t meta_bytes = 0;
    sora_frame_result* d_tmpl = nullptr; size_t tmpl_bytes = 0;
};
void sora_internal_dense_free(DenseStage* D);
int sora_internal_dense_deliver(DenseStage* D, const sora::Rx11bRow* d_rows, const uint32_t* d_nframes, const sora::CapDesc* d_caps, const sora_frame_result* h_tmpl,
                                uint32_t ncaps, uint32_t mf, const uint8_t* d_slots, hipStream_t st,
                                sora_frame_result* h_rows, size_t max_rows, uint32_t* h_meta, uint8_t* h_mpdu, size_t mpdu_cap,
                                // (a template already on the device; the real number of "captures" where the host
                                // only knows a bound; per "capture" the row its rows start at, k_dense_rows)
                                const sora_frame_result* d_tmpl = nullptr, const uint32_t* d_ncaps = nullptr, const uint32_t* d_evbase = nullptr);
// k_deliver.hip: *_results / *_results_of of the same handles on the host -- rows and MPDUs of a call whose captures were caps[0, ncaps), behind its stream
int sora_internal_rows_results(const sora::Rx11bRow* d_rows, const uint32_t* d_nframes, const uint8_t* d_mpdu, const sora_capture_desc* caps, uint32_t ncaps, uint32_t mf,
                               int device, hipStream_t st, const char* who, sora_frame_result* out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap);

// sora_hip.cpp: the i-th stream of a handle (its i-th pipeline / slot), non-blocking, on priority level i % 3: the runtime keeps GPU_MAX_HW_QUEUES
// hardware queues per level, so a handle's streams get a hardware queue each without the application setting an environment variable
hipError_t sora_internal_stream_create(hipStream_t* out, int index);
// sora_hip.cpp: records the message sora_hip_last_error() returns; hip_error = 0 for none
int sora_internal_fail(int code, const char* what, int hip_error);
const uint32_t* sora_internal_crc_table(int device);
struct sora_rx;
extern "C" int sora_internal_rx_device(sora_rx* rx);                           // device ordinal of a receive handle (sora_shard.cpp)
int sora_internal_tables(int device, sora::Tables* out);                  // the per-device tables of the stage entry points (uploaded on first use)
void sora_internal_dsp_host_tables(std::vector<uint32_t>& sincos, std::vector<short>& atan);   // k_11n.hip: the two dsp_math tables as the host generates them
int sora_internal_pin_table(const char* name, const void* data, size_t bytes);   // sora_hip.cpp: SORA_OK iff the bytes are the pinned sha256 of table `name`
// dsp_math tables of the current device (k_11n.hip)   // device pointer to the 256-entry CRC-32 table of `device` (uploaded on first use), or nullptr
int sora_internal_dsp_tables(const uint32_t** sincos, const short** atan);
