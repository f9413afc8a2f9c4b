// k_rx11n.hip -- the reference's 802.11n 2x2 receive graph over a batch of independent two-chain captures:
// CreateDemodGraph11n (kernel/bb/demod11/fb11ndemod_config.hpp:166-257) driven as RxThread drives it (fb11n_demod.cpp:30-85).
//
//   TMemSamples2 -> TDownSample2 -> RxSwitch -> TCCA11n (MimoAutoCorr)                                   carrier sense
//                                            -> TFreqEstimator_11n -> TFreqComp_11n -> TFFT64 x4 -> TSisoChannelEst    L-LTF
//                                            -> TFreqComp_11n -> T11nDataSymbol -> TFFT64 x2 -> T11nSymSel
//       SIG:    TSisoChannelComp -> TMrcCombine -> T11nSigDemap -> T11aDeinterleaveBPSK -> T11nViterbiSig -> T11nSigParser
//       HT-LTF: TMimoChannelEst
//       DATA:   TMimoChannelComp -> TPilotTrack_11n -> T11nDemap* -> T11nDeinterleave*_S0/_S1 -> TStreamJoin -> TStreamConcat<2,1>
//               -> T11aViterbi<5000*8, 312, 192, 36> -> T11aDesc -> TBB11aFrameSink
//
// One wave per capture (four per workgroup); all control flow is wave-uniform, the 64 lanes are the 64 samples / carriers / trellis
// states of the step at hand.  The graph's queues reduce to positions in the 20 MHz stream:
//   * a source call brings 14 samples; a frame event is seen when the call that completed its last burst returns, the queues are
//     cleared and the stream restarts at the next call boundary;
//   * carrier sense runs in blocks of 64 samples: the moving sums are prefix sums over the lanes on top of the rings MimoAutoCorr
//     keeps, the peak counter walks the two ballots of its conditions;
//   * TFreqComp_11n's running phase is n * CFO - theta (mod 2^16) for the n-th sample after detection;
//   * samples past the end of the capture read as zero: that is the flush TMemSamples2 issues when it runs dry, which pads every
//     partly filled queue with zero items (see oracle/so_rx11n.c, flush_graph).
// HBM traffic = the samples, once (8 bytes per 40 MHz sample pair of the two chains, of which the even half is used).
#include "kernels.h"
#include "dev_winplan.h"
#include "dev_11n.h"
#include "../../include/sora_hip.h"
#include <type_traits>

namespace sora {

struct Rx11nArgs {
    const uint32_t* iq0; const uint32_t* iq1;    // packed COMPLEX16 @40 MHz, RX chain 0 / 1
    const CapDesc*  caps; uint32_t ncaps, max_frames;
    Rx11bRow*       rows;                          // [ncaps * max_frames]: end_sample = 40 MHz source position, rate_kbps = MCS index
    uint32_t*       nframes;                       // [ncaps]
    uint8_t*        mpdu;                          // [ncaps * max_frames][4096]
    Tables          T;
    const uint32_t* sincos; const short* atan;     // dsp_math tables
};

namespace {
__device__ __forceinline__ unsigned long long uni64(unsigned long long v)
{
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ int scan_add(int v, int)                    // inclusive prefix sum over the wave, wrapping: six DPP adds, no LDS round trips
{
    // inside each row of 16: row_shr:1, 2, 4, 8 (lanes shifted in read 0); then lane 15 of row r - 1 into rows 1 and 3, lane 31 into rows 2 and 3
    v = (int)((unsigned)v + (unsigned)__builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true));
    v = (int)((unsigned)v + (unsigned)__builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true));
    v = (int)((unsigned)v + (unsigned)__builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true));
    v = (int)((unsigned)v + (unsigned)__builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true));
    v = (int)((unsigned)v + (unsigned)__builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false));   // row_bcast:15, rows 1 and 3
    v = (int)((unsigned)v + (unsigned)__builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false));   // row_bcast:31, rows 2 and 3
    return v;
}
}  // namespace

// ================================================================================================================================
// The 802.11n graph as a chain of kernels, the way the 802.11a path is built (k_scan -> k_frame -> k_viterbi -> k_finish):
//   k_scan11n     one wave per capture: carrier sense, L-LTF (CFO, four FFTs, TSisoChannelEst), the three SIG symbols and their decoder,
//                 RxThread's bookkeeping.  What follows the SIG field never feeds back into carrier sense -- the event of a frame is
//                 raised at its last data symbol, whose position the SIG field fixes (T11nSymSel counts remain_symbols down,
//                 PHY_11n.hpp:331; equivalently the Viterbi passes frame_length * 8 + 22 steps in that symbol) -- so the scan jumps
//                 over the data field and queues it as a job: (capture, L-LTF position, CFO, MCS, length, symbols, soft values incl.
//                 the zero padding of a flush at the end of the capture).
//   k_frame11n    one wave per queued frame: the two HT-LTF symbols -> TMimoChannelEst, then symbol by symbol (the pilot phase of
//                 symbol s rotates symbol s + 1: a serial chain) TFreqComp_11n, two FFTs, TMimoChannelComp, TPilotTrack_11n, demap,
//                 de-interleave, stream join; soft values leave as the 16-bit fields v << 9 the trellis kernel reads.
//   k_viterbi11n  k_rx.hip: the two-frames-per-wave trellis kernel of the 802.11a path with the 192 / 36 window schedule.
//   k_finish11n   T11aDesc + TBB11aFrameSink: descrambler phase table, parallel CRC-32; fills error code, FCS and the MPDU slot of the row.
struct N11Frame {                  // one queued data field
    uint32_t cap;                  // capture index
    uint32_t row;                  // index into rows[] / mpdu slots
    uint32_t l0;                   // 20 MHz index (in the capture) of the first L-LTF sample
    int32_t  cfo;
    uint32_t mcs, ht_len, code_rate;
    uint32_t nproc;                // data symbols that start inside the (padded) capture
    uint32_t nsoft;                // soft values handed to the decoder, zero padding of a final flush included
    uint32_t slot0;                // first symbol slot (global) of the frame's soft / decoded-byte storage
    uint32_t pad[6];
};
struct Scan11nArgs {
    const uint32_t* iq0; const uint32_t* iq1; const CapDesc* caps; uint32_t ncaps, max_frames;
    Rx11bRow* rows; uint32_t* nframes; Tables T; const uint32_t* sincos; const short* atan;
    N11Frame* frames;              // [3][nrows], by code-rate list, compacted
    VitJob*   jobs;                // [3][nrows], same order
    uint32_t* njobs;               // [3]
    uint32_t  nrows;
    // sora_rx11n_set_mcs_max: the highest MCS the SIG parser accepts (10 = PHY_11n.hpp:497), and the handle's bytes per symbol slot (soft values / decoded bytes)
    uint32_t  mcs_max, soft_per_slot, out_per_slot;
    uint32_t  joint;               // HT40 only: 1 = the handle's coding is the joint one (sora_ht40_set_coding): a frame's N_DBPS spans both streams
    uint32_t  guard;               // HT40 only: 1 = SORA_HT40_GUARD_SIGNALLED (sora_ht40_set_guard): the host launches the forms that read HT-SIG's Short GI bit
};
// A symbol slot of the 802.11n handle: kSoftPerSlot / kOutPerSlot (rx_types.h) while the gate stands at MCS 10 (208 soft values, 19.5 decoded bytes per symbol at
// most); with the gate raised a symbol brings up to 624 soft values and 58.5 decoded bytes (MCS 14)
constexpr uint32_t kSoftPerSlot11nWide = 640, kOutPerSlot11nWide = 64;
struct Frame11nArgs {
    const uint32_t* iq0; const uint32_t* iq1; const CapDesc* caps;
    const N11Frame* frames; const uint32_t* njobs; uint32_t nrows;
    Tables T; const uint32_t* sincos; const short* atan;
    uint8_t* soft;                 // [slots * 288] the frames' soft streams, one byte per value (VitJob::soft_bits = 8)
    VitJob*   jobs;                // [3][nrows]: k_frame11n fills in the pair stream's offset (the mate is known only after the scan)
    const uint8_t* vout;           // [slots * 32]
    Rx11bRow* rows; uint8_t* mpdu;
    uint32_t soft_per_slot, out_per_slot;
};

namespace {
struct ScanLds {
    uint32_t his[2][32]; int hcr[2][32], hci[2][32], he[2][32];
    long long his_e[64];
    uint32_t buf[2][128];
    uint32_t fft[4][64];
    uint32_t y[2][128];
    uint32_t ch[2][64];
    uint32_t sig[192];
    uint8_t  soft0[160];
    uint8_t  sigsoft[144];
    unsigned long long dec[52];
};
struct FrameLds {
    uint32_t buf[2][64];
    uint32_t fft[4][64];
    uint32_t y[2][128];
    uint32_t hinv[4][64];
    uint32_t xs[2][64];
    uint8_t  soft[2][320];         // the two streams' demapped symbol: up to 52 x 6 values each
};
// stream continuation (sora_rx11n_set_stream_mode): the carrier-sense rings at the latest resume point in front of a detection (k_scan11n_stream)
struct RingLds {                   // the same layout as the head of ScanLds
    uint32_t his[2][32]; int hcr[2][32], hci[2][32], he[2][32];
    long long his_e[64];
};
constexpr uint32_t kRec11nMagic = 0x534F314Eu;     // a continuation record holds a resume point (a fresh stream is all zeros)
}  // namespace

// HT40 = false: the reference's 20 MHz graph (k_scan11n).  HT40 = true: the same front end on the legacy part of an HT-mixed 40 MHz frame
// (k_scan_ht40): the legacy preamble and HT-SIG are the 20 MHz waveforms sent on both halves of the channel, the upper one rotated by
// 90 degrees, so the even samples of x[n] j^n -- (-1)^m x[2m]: a sign per sample -- are (1 + j) times the 20 MHz legacy waveform and
// every brick up to T11nSigParser applies unchanged (oracle/py_ht40.py tx_frame / front_end_view; tests/test_ht40_preamble_model.py
// runs the restated reference receiver on it).  What differs behind the parser: MCS 8..14 at CBW 40 and lengths up to 4000 are
// accepted (PHY_11n.hpp:497 accepts 8..10 at 1500), and instead of queueing a 20 MHz data field the frame is recorded for the 40 MHz
// data-field kernels (k_ht40.hip) with what they need from here: position, CFO (per 40 MHz sample) and the noise variance, estimated
// from the difference of the two L-LTF symbols.  That part is this library's own definition: parity unpinned.
//
// STREAM = true (k_scan11n_stream / k_scan_ht40_stream, sora_rx11n_set_stream_mode / sora_ht40_set_stream_mode): the capture continues the stream its continuation record
// left off.  A RESUME POINT is a burst boundary of carrier sense that falls on a source-call boundary: 28 samples (20 MHz) apart from each
// origin, and every post-event origin.  The record: [0] kRec11nMagic, [1] ring_pos, [2] his_index, [3..8] the running sums, [9..12] the
// TCCA11n counters pf, pc, sense, timeout, then the rings in their LDS layout.  Three things differ from the default kernel:
//   * carrier-sense blocks are 56 samples, so every block starts at a resume point, and carrier sense stops at the last resume point of the
//     capture (a detection behind it cannot complete its L-LTF and SIG inside the capture);
//   * a frame is taken only when all of its symbols lie inside the capture (no flush: a capture's end is not the stream's end), and only when
//     it finds a row slot; else the capture ends at the latest resume point in front of its detection.  That point is the detecting block's
//     start or its middle (sample 28): at the detection, before the block's ring writes, the rings as they stand there -- the block's own
//     samples in front of it, the block-start values behind -- go to an LDS copy with the sums and counters of that point.  That costs one
//     copy per detection and nothing per block, and it is exact: nothing but the block's writes moved the rings since the block started;
//   * the record is written once, at the end of the capture, from the rings or their copy (a zero-length capture leaves it as it was).
// Every addition sits under "if constexpr (STREAM)": the default kernels are the instruction stream they were.
// GI = true (HT40 only: k_scan_ht40_gi / k_scan_ht40_stream_gi, launched for a handle in SORA_HT40_GUARD_SIGNALLED): HT-SIG bit 31 (Short GI) of a
// sound header is read; a frame that sets it has data symbols of 72 samples at 20 MHz and its record carries SORA_HT40_SHORT_GI on the MCS.  With the bit clear, and in the
// forms without GI, nothing differs.
template <bool HT40, bool STREAM = false, bool GI = false>
__device__ __forceinline__ void scan11n_body(const Scan11nArgs& A, Ht40Found* found, uint32_t* cont = nullptr, uint32_t* consumed = nullptr)
{
    __shared__ ScanLds s_w[4];
    __shared__ uint8_t s_lut[6][256];
    fill_demap_luts(s_lut);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t cap = blockIdx.x * 4 + wv;
    if (cap >= A.ncaps) return;
    ScanLds& W = s_w[wv];
    const CapDesc cd = A.caps[cap];
    const uint32_t* iq[2] = { A.iq0 + cd.offset, A.iq1 + cd.offset };
    const uint32_t n20 = cd.nsamples / 2;
    // HT40: the derotation sign goes by i & 1, the 20 MHz index counted from the capture's first sample.  A continued capture (STREAM) starts at a resume
    // point: a multiple of 28 samples at 40 MHz, that is 14 k at 20 MHz from the previous capture's start -- an even number.  So the sign pattern runs on
    // unbroken from call to call, the rings in the continuation record hold derotated samples of the same phase, and the host's "continue from the resume
    // point" rule needs no alignment rule of its own for the 40 MHz front end.
    auto fetch = [&](int r, uint32_t i) __attribute__((always_inline)) -> uint32_t {
        if (i >= n20) return 0u;
        const uint32_t v = iq[r][2 * (size_t)i];
        if (HT40 && (i & 1u)) { const cpx c = unpack(v); return pack(mk(sat16(-c.re), sat16(-c.im))); }     // x[2m] (-1)^m
        return v;
    };
    const Fft64Tw tw = fft64_twiddles(A.T, lane & 15);

    int sr[2] = { 0, 0 }, si[2] = { 0, 0 }, se[2] = { 0, 0 };
    int ring_pos = 0, his_index = 0;
    // stream mode: the counters the next carrier sense starts from, the state at the latest resume point in front of a detection (sv_*, RingLds),
    // and where the capture ends
    RingLds* SV = nullptr;
    uint32_t* const rec = STREAM ? cont + (size_t)cap * kRec11nWords : nullptr;
    int ld_pf = 0, ld_pc = 0, ld_sense = 0, ld_to = 0;
    int sv_ring = 0, sv_hisi = 0, sv_sr[2] = { 0, 0 }, sv_si[2] = { 0, 0 }, sv_se[2] = { 0, 0 }, sv_pf = 0, sv_pc = 0, sv_sense = 0, sv_to = 0;
    uint32_t sv_pos = 0, fin_pos = 0; bool saved = false, fin = false;
    bool fresh = true;
    if constexpr (STREAM) {
        __shared__ RingLds s_sv[4];
        SV = &s_sv[wv];
        const uint32_t h = rec[lane];
        if ((uint32_t)__builtin_amdgcn_readlane((int)h, 0) == kRec11nMagic) {
            fresh = false;
            auto w = [&](int k) __attribute__((always_inline)) { return __builtin_amdgcn_readlane((int)h, k); };
            ring_pos = w(1); his_index = w(2); sr[0] = w(3); sr[1] = w(4); si[0] = w(5); si[1] = w(6); se[0] = w(7); se[1] = w(8);
            ld_pf = w(9); ld_pc = w(10); ld_sense = w(11); ld_to = w(12);
            const uint32_t* rw = rec + 64;
            W.his[lane >> 5][lane & 31] = rw[lane]; W.hcr[lane >> 5][lane & 31] = (int)rw[64 + lane];
            W.hci[lane >> 5][lane & 31] = (int)rw[128 + lane]; W.he[lane >> 5][lane & 31] = (int)rw[192 + lane];
            W.his_e[lane] = reinterpret_cast<const long long*>(rec + 64 + 256)[lane];
        }
    }
    if (fresh)
    for (int k = lane; k < 64; k += 64) { W.his[0][k & 31] = 0; W.his[1][k & 31] = 0; W.hcr[k >> 5][k & 31] = 0; W.hci[k >> 5][k & 31] = 0;
        W.he[k >> 5][k & 31] = 0; W.his_e[k] = 0x7FFFFFFFFFFFFFFFll; }
    wave_lds_sync();
    uint32_t origin = 0, nfr = 0;
    Rx11bRow* rows = A.rows + (size_t)cap * A.max_frames;

    while (origin < n20) {
        // ================================================================ carrier sense from `origin` (cca_11n.hpp:46-127)
        const uint32_t nb_total = (n20 - origin + 3) / 4;
        bool pf = false, timeout = false; int pc = 0, sense = 0;
        // stream mode: 56-sample blocks, up to the capture's last resume point
        constexpr uint32_t kBlk = STREAM ? 56u : 64u;
        const uint32_t cs_end = STREAM ? (n20 - origin) / 28 * 28 : nb_total * 4;
        bool b_pf = false, b_to = false; int b_pc = 0, b_sense = 0, c_pf = 0, c_pc = 0, c_sense = 0, c_to = 0;
        if constexpr (STREAM) { pf = ld_pf != 0; pc = ld_pc; sense = ld_sense; timeout = ld_to != 0; ld_pf = ld_pc = ld_sense = ld_to = 0; }
        int64_t det_at = -1;
        for (uint32_t base = 0; base < cs_end && det_at < 0; base += kBlk) {
            const int lim = (int)min(kBlk, cs_end - base);
            if constexpr (STREAM) { b_pf = pf; b_pc = pc; b_sense = sense; b_to = timeout; }
            int pr[2], pi[2], pe[2], cre[2], cim[2], een[2]; uint32_t xr[2];
            const int slot = (ring_pos + lane) & 31;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                xr[r] = fetch(r, origin + base + lane);
                const cpx x = unpack(xr[r]);
                const uint32_t dl = (uint32_t)__shfl((int)xr[r], lane - 32);
                const cpx delayed = unpack(lane < 32 ? W.his[r][slot] : dl);
                int re, im; conj_mul32(x, delayed, re, im); re >>= 5; im >>= 5;
                const int ore = __shfl(re, lane - 32), oim = __shfl(im, lane - 32);
                const int e = sqnorm(x) >> 5, oe = __shfl(e, lane - 32);
                const int dre = (int)((unsigned)re - (unsigned)(lane < 32 ? W.hcr[r][slot] : ore));
                const int dim = (int)((unsigned)im - (unsigned)(lane < 32 ? W.hci[r][slot] : oim));
                const int den = (int)((unsigned)e - (unsigned)(lane < 32 ? W.he[r][slot] : oe));
                pr[r] = (int)((unsigned)sr[r] + (unsigned)scan_add(dre, lane)); pi[r] = (int)((unsigned)si[r] + (unsigned)scan_add(dim, lane));
                pe[r] = (int)((unsigned)se[r] + (unsigned)scan_add(den, lane));
                cre[r] = re; cim[r] = im; een[r] = e;
            }
            const int are = (int)((unsigned)(pr[0] >> 1) + (unsigned)(pr[1] >> 1)), aim = (int)((unsigned)(pi[0] >> 1) + (unsigned)(pi[1] >> 1));
            const long long acorr = (long long)((unsigned long long)((long long)are * are) + (unsigned long long)((long long)aim * aim));
            const int ev = (int)((unsigned)(pe[0] >> 1) + (unsigned)(pe[1] >> 1));
            const long long energy = (long long)ev * ev;
            const long long olde = W.his_e[(his_index + lane) & 63];
            const bool cA = olde != 0x7FFFFFFFFFFFFFFFll && (olde + 1) <= (energy >> 2) && 6 * (olde + 1) <= energy && acorr > (energy >> 1);
            const bool cB = acorr < (energy >> 3);
            const unsigned long long bA = __ballot(cA), bB = __ballot(cB);
            int det = -1;
            const unsigned long long lmask = lim >= 64 ? ~0ull : ((1ull << lim) - 1);
            if (!pf && (bA & lmask) == 0) {
                // idle block: per 4-sample burst j  sense += 4; sense >= 84 raises the time-out; a raised time-out is cleared, with the counter, by
                // the first burst that ends a 14-sample source call.  In closed form over the block's bursts (sense needs 21 bursts to reach 84:
                // at most one time-out is raised inside a block): lane j says whether burst j ends a source call, two find-first-bits do the rest.
                const int nbst = lim >> 2;
                const uint32_t X = (uint32_t)__ballot(((base + 4u * (uint32_t)lane + 3u) % 14u) >= 10u) & (nbst >= 32 ? 0xFFFFFFFFu : ((1u << nbst) - 1u));
                int j = 0;
                bool counted = false;
                if (timeout) {
                    if (X == 0u) { sense += 4 * nbst; counted = true; }
                    else { j = __builtin_ctz(X) + 1; sense = 0; timeout = false; }
                }
                if (!counted) {
                    const int r = nbst - j, k = max((84 - sense + 3) >> 2, 1);          // bursts left in the block; bursts until the counter reaches 84
                    if (k > r) sense += 4 * r;
                    else {
                        const int jt = j + k - 1;                                       // the burst that raises the time-out (it may clear it itself)
                        const uint32_t m = jt >= 32 ? 0u : (X >> jt) << jt;
                        if (m == 0u) { sense += 4 * r; timeout = true; }
                        else { sense = 4 * (nbst - 1 - __builtin_ctz(m)); timeout = false; }
                    }
                }
                pc = 0;
            } else if (pf && !timeout && (bB & lmask) == 0 && pc + lim <= 160) {
                pc += lim;
            } else
            for (int i = 0; i < lim; i++) {
                const bool a = (bA >> i) & 1, b = (bB >> i) & 1;
                if (!pf) { sense++; if (a) { sense = 0; pc++; pf = true; } else pc = 0; }
                else if (b) { const bool good = pc > 96 && pc < 160; pf = false; pc = 0; if (good) { det = i; break; } }
                else { pc++; if (pc > 160) { pf = false; pc = 0; } }
                if ((i & 3) == 3) {
                    if (sense >= 84) timeout = true;
                    const uint32_t s4 = base + (uint32_t)i - 3;
                    if (timeout && (s4 + 3) / 14 != (s4 + 7) / 14) { timeout = false; pf = false; pc = 0; sense = 0; }
                }
                if constexpr (STREAM) if (i == 27) { c_pf = pf; c_pc = pc; c_sense = sense; c_to = timeout; }   // the block's middle resume point
            }
            const int ne = det >= 0 ? det : lim;
            const int na = det >= 0 ? (det | 3) + 1 : lim;
            if constexpr (STREAM) {
                if (det >= 0) {
                    // the latest resume point in front of the detecting burst: the block's start (m = 0) or its middle (m = 28).  The rings there:
                    // slot ring_pos + j (j < 32) holds lane j's sample if j < m, else what it held when the block started
                    const int m = (det & ~3) >= 28 ? 28 : 0;
                    if (lane < 32) {
#pragma unroll
                        for (int r = 0; r < 2; r++) {
                            SV->his[r][slot] = lane < m ? xr[r] : W.his[r][slot]; SV->hcr[r][slot] = lane < m ? cre[r] : W.hcr[r][slot];
                            SV->hci[r][slot] = lane < m ? cim[r] : W.hci[r][slot]; SV->he[r][slot] = lane < m ? een[r] : W.he[r][slot];
                        }
                    }
                    SV->his_e[(his_index + lane) & 63] = lane < m ? energy : olde;
                    sv_ring = (ring_pos + m) & 31; sv_hisi = (his_index + m) & 63;
#pragma unroll
                    for (int r = 0; r < 2; r++) {
                        sv_sr[r] = m ? __shfl(pr[r], 27) : sr[r]; sv_si[r] = m ? __shfl(pi[r], 27) : si[r]; sv_se[r] = m ? __shfl(pe[r], 27) : se[r];
                    }
                    sv_pf = m ? c_pf : b_pf; sv_pc = m ? c_pc : b_pc; sv_sense = m ? c_sense : b_sense; sv_to = m ? c_to : b_to;
                    sv_pos = origin + base + (uint32_t)m;
                }
            }
            if (lane < ne) W.his_e[(his_index + lane) & 63] = energy;
            if (lane < na && lane >= na - 32) {
#pragma unroll
                for (int r = 0; r < 2; r++) { W.his[r][slot] = xr[r]; W.hcr[r][slot] = cre[r]; W.hci[r][slot] = cim[r]; W.he[r][slot] = een[r]; }
            }
#pragma unroll
            for (int r = 0; r < 2; r++) { sr[r] = __shfl(pr[r], na - 1); si[r] = __shfl(pi[r], na - 1); se[r] = __shfl(pe[r], na - 1); }
            his_index = (his_index + ne) & 63; ring_pos = (ring_pos + na) & 31;
            wave_lds_sync();
            if (det >= 0) det_at = (int64_t)base + na;
        }
        if constexpr (STREAM) if (det_at < 0) { ld_pf = pf; ld_pc = pc; ld_sense = sense; ld_to = timeout; fin_pos = origin + cs_end; fin = true; }
        if (det_at < 0) break;
        const uint32_t n_real = n20 - origin;
        const uint32_t n_pad = (n_real + 3) & ~3u;                           // the last burst is delivered zero-padded
        const uint32_t l0 = (uint32_t)det_at;
        // stream mode: the L-LTF and the three SIG symbols inside the capture, and a row slot for the event every such frame raises; else the
        // capture ends in front of the detection
        if constexpr (STREAM) if (l0 + 128 + 240 > n_real || nfr >= A.max_frames) { saved = true; break; }
        if (l0 + 128 > n_pad) break;
        // ================================================================ L-LTF: CFO, compensation, four FFTs, SISO channel
        const int cfo = uni(cfo_est11n(A.atan, unpack(fetch(0, origin + l0 + lane)), unpack(fetch(0, origin + l0 + 64 + lane)),
                                       unpack(fetch(1, origin + l0 + lane)), unpack(fetch(1, origin + l0 + 64 + lane))));
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int n = 64 * h + lane;
                const cpx cof = unpack(A.sincos[(unsigned)(n * cfo) & 0xFFFFu]);
                W.buf[r][n] = pack(freq_comp11n(unpack(fetch(r, origin + l0 + n)), cof));
            }
        wave_lds_sync();
        {
            const int g = lane >> 4, e = lane & 15; cpx x[4], yy[4];
#pragma unroll
            for (int m = 0; m < 4; m++) x[m] = unpack(W.buf[g >> 1][64 * (g & 1) + e + 16 * m]);
            fft64_group(x, yy, W.fft[g], e, tw, wave_lds_sync);
#pragma unroll
            for (int q = 0; q < 4; q++) W.y[g >> 1][64 * (g & 1) + e + 16 * q] = pack(yy[q]);
        }
        wave_lds_sync();
        float noise_var = 0.0f;
        // the two L-LTF symbols differ by noise only: E|Y1 - Y2|^2 = 2 var(FFT<64> bin); an FFT<128> bin of the
        if (HT40) {
            // 40 MHz stream carries half that (same noise per sample, twice the 1/N), so noise_var = sum / (4 x 104 bins)
            float acc = 0.0f;
            if (lane != 0 && (lane < 27 || lane >= 38)) {
#pragma unroll
                for (int r = 0; r < 2; r++) {
                    const cpx p = unpack(W.y[r][lane]), q = unpack(W.y[r][64 + lane]);
                    const float dr = (float)(p.re - q.re), di = (float)(p.im - q.im);
                    acc += dr * dr + di * di;
                }
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
            noise_var = acc * (1.0f / 416.0f);
        }
#pragma unroll
        for (int r = 0; r < 2; r++) W.ch[r][lane] = siso_est_carrier(W.y[r], lane);
        wave_lds_sync();
        // ================================================================ the SIG field: three symbols, theta = 0 (no pilot tracking before the data field)
        uint32_t err = 0, mcs = 0, ht_len = 0, code_rate = 0;
        [[maybe_unused]] uint32_t sgi = 0;                                   // GI: HT-SIG bit 31 of a header that passed the gate
        bool sig_ok = false, decoded = false;
        uint32_t a = l0 + 128;
        int nsig = 0;
        bool at_end = false;
        for (int s3 = 0; s3 < 3; s3++) {
            if (a >= n_pad) { at_end = true; break; }
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const uint32_t n = a - l0 + 16 + lane;
                const cpx cof = unpack(A.sincos[(unsigned)((int)n * cfo) & 0xFFFFu]);
                W.buf[r][lane] = pack(freq_comp11n(unpack(fetch(r, origin + a + 16 + lane)), cof));
            }
            wave_lds_sync();
            {
                const int g = lane >> 4, e = lane & 15; cpx x[4], yy[4];
#pragma unroll
                for (int q = 0; q < 4; q++) x[q] = unpack(W.buf[g & 1][e + 16 * q]);
                fft64_group(x, yy, W.fft[g], e, tw, wave_lds_sync);
                if (g < 2) {
#pragma unroll
                    for (int q = 0; q < 4; q++) W.y[g][e + 16 * q] = pack(yy[q]);
                }
            }
            wave_lds_sync();
            {
                cpx x0, x1;
                W.sig[64 * nsig + lane] = pack(siso_comp_mrc(unpack(W.y[0][lane]), unpack(W.ch[0][lane]), unpack(W.y[1][lane]), unpack(W.ch[1][lane]), x0, x1));
            }
            nsig++; a += 80;
            wave_lds_sync();
        }
        // T11nSymSel::Flush: the missing symbols are zeros
        if (at_end && nsig > 0) { for (int k = lane; k < 64 * (3 - nsig); k += 64) W.sig[64 * nsig + k] = 0; }
        if (!at_end || nsig > 0) {
            // T11nSigDemap -> T11aDeinterleaveBPSK -> T11nViterbiSig -> T11nSigParser on W.sig
            decoded = true;
            wave_lds_sync();
            for (int g = lane; g < 144; g += 64) {
                const int s3 = g / 48, k = g - 48 * s3;
                W.soft0[g] = sig_demap_soft(unpack(W.sig[64 * s3 + carrier_bin48(k)]), s3, s_lut);
            }
            wave_lds_sync();
            for (int g = lane; g < 144; g += 64) { const int s3 = g / 48, kk = g - 48 * s3; W.sigsoft[g] = W.soft0[48 * s3 + sig_deint_index(kk)]; }
            wave_lds_sync();
            const uint32_t lsig = (uint32_t)uni((int)(uint32_t)(viterbi_sig_wave<24>(W.sigsoft, reinterpret_cast<uint64_t*>(W.dec), lane) >> 6));
            wave_lds_sync();
            const unsigned long long ht = uni64(viterbi_sig_wave<48>(W.sigsoft + 48, reinterpret_cast<uint64_t*>(W.dec), lane) >> 6);
            wave_lds_sync();
            const SigFront P = sig_parse_front(lsig, ht);
            // the gate.  HT40: two streams, 40 MHz, up to the handle's mcs_max (14, or 15 after sora_ht40_set_mcs_max); else mcs_max (10: the reference's ht_frame_mcs >= 11) and 1500 bytes
            if (HT40) sig_ok = P.ok && P.mcs >= 8 && P.mcs <= A.mcs_max && P.cbw40 && P.ht_len <= 4000 && P.ht_len >= 4;
            else sig_ok = P.ok && P.mcs >= 8 && P.mcs <= A.mcs_max && P.ht_len <= 1500;
            if (sig_ok) { mcs = P.mcs; ht_len = P.ht_len; code_rate = HT40 ? code_rate_ht40(P.mcs) : code_rate11n(P.mcs); if constexpr (GI) sgi = (uint32_t)(ht >> 31) & 1u; }
            else err = E_PLCP_HEADER_FAIL;
        }
        // ================================================================ what happens to the frame, without looking at its data field
        uint32_t last_burst_end = n_pad;                                     // (relative to origin) behind the burst that raises the event
        bool event = false, queue = false;
        uint32_t nproc = 0, nsoft = 0;
        if (decoded && err != 0) { event = true; last_burst_end = at_end ? n_pad : min(a, n_pad); }
        else if (HT40 && decoded && !at_end) {
            // HT-STF at a, HT-LTF 1 / 2 at a + 80 / a + 160, data symbol d at a + 240 + 80 d (20 MHz indices; 4 us symbols).  The frame is
            // recorded when all of it lies inside the capture; a frame the capture cuts off raises no event (as the 20 MHz graph behaves).
            const uint32_t ndbps = ht40_ndbps(nbpsc11n(mcs), code_rate) << A.joint;
            const uint32_t nsym = (16u + 8u * ht_len + 6u + ndbps - 1u) / ndbps;
            nproc = nsym;
            if constexpr (GI) {
                // (Short GI: data symbol d at a + 240 + 72 d, 3.6 us symbols)
                const uint32_t end = a + 240 + (sgi ? 72u : 80u) * nsym;
                // (stream form: a short frame is taken when the kHt40ShortAdvance samples k_ht40_plan moves its data field by lie inside the piece too, so that every
                // cut of a stream gives the one-call result; else the next call finds it)
                if (end + ((STREAM && sgi) ? kHt40ShortAdvance / 2u : 0u) <= n_real) { event = true; queue = true; last_burst_end = end; }
            }
            else
            if (a + 240 + 80 * nsym <= n_real) { event = true; queue = true; last_burst_end = a + 240 + 80 * nsym; }
        }
        else if (decoded && !at_end) {
            // HT-STF at a, HT-LTF at a + 80 / a + 160, data symbol d at a + 240 + 80 d; a symbol is processed when it starts inside the
            // padded capture (its missing samples read as zero: the flush of the partly filled queues)
            const uint32_t tr_end = ht_len * 8 + 16 + 6;
            const uint32_t S = 104u * nbpsc11n(mcs), sps = data_bits11n(S, code_rate);     // soft values / trellis steps per symbol
            const uint32_t nsym = (tr_end + sps - 1) / sps;                  // the symbol in which the decoder passes tr_end
            const uint32_t a_data = a + 240;
            if constexpr (STREAM) {                                          // all of the data field inside the capture, or no event (and no flush)
                if (a_data + 80 * nsym <= n_real) { nproc = nsym; event = true; queue = true; nsoft = nsym * S; last_burst_end = a_data + 80 * nsym; }
            }
            else {
            if (a_data < n_pad) nproc = min(nsym, (n_pad - a_data + 79) / 80);
            if (nproc == nsym) { event = true; queue = true; nsoft = nsym * S; last_burst_end = min(a_data + 80 * nsym, n_pad); }
            else if (a + 160 < n_pad && nproc > 0 && (nproc * S) % 312 != 0) {
                // the capture ends inside the data field: T11aViterbi's 312-value input burst is padded with zero soft values; an
                // event only if that takes the decoder past tr_end.  (64-QAM: a symbol is two whole bursts, the decoder holds nothing back and
                // a cut frame raises no event; 16-QAM: a symbol is a burst and a third, as QPSK's is two thirds.)
                nsoft = (nproc * S + 311) / 312 * 312;
                const uint32_t steps = data_bits11n(nsoft, code_rate);
                if (steps >= tr_end) { event = true; queue = true; last_burst_end = n_pad; }
            }
            }
        }
        if constexpr (STREAM) if (!event) { saved = true; break; }          // the frame runs past the capture: the next call finds it
        if (!event) break;                                                   // the capture ended inside a frame without an event
        const uint32_t abs_end = origin + last_burst_end;
        const uint32_t call = (abs_end - 1) / 14;
        const uint32_t next = min(14 * (call + 1), n20);
        if (nfr < A.max_frames) {
            const uint32_t row = cap * A.max_frames + nfr;
            if (lane == 0) {
                Rx11bRow r; r.end_sample = 2 * next; r.error_code = queue ? 0u : err; r.rate_kbps = queue ? mcs : 0u; r.length = queue ? ht_len : 0u; r.crc32 = 0u;
                rows[nfr] = r;
                if (HT40) {
                    Ht40Found F; F.a20 = origin + a; F.mcs = queue ? mcs : 0u; F.ht_len = queue ? ht_len : 0u; F.cfo = cfo; F.noise_var = noise_var;
                    if constexpr (GI) { if (queue && sgi) F.mcs |= SORA_HT40_SHORT_GI; }
                    F.end_sample = 2 * next; F.error_code = queue ? 0u : err; F.nsym = queue ? nproc : 0u;
                    found[row] = F;
                } else if (queue) {
                    const uint32_t list = code_rate;
                    const uint32_t idx = atomicAdd(&A.njobs[list], 1u);
                    N11Frame F; F.cap = cap; F.row = row; F.l0 = origin + l0; F.cfo = cfo; F.mcs = mcs; F.ht_len = ht_len; F.code_rate = code_rate;
                    F.nproc = nproc; F.nsoft = nsoft; F.slot0 = cd.slot_base + (origin + a + 240) / 80;
                    for (int k = 0; k < 6; k++) F.pad[k] = 0;
                    A.frames[(size_t)list * A.nrows + idx] = F;
                    VitJob J; J.soft_off = F.slot0 * A.soft_per_slot; J.soft_bits = 8; J.nsoft = nsoft; J.length = ht_len; J.dec_off = 0;
                        J.out_off = F.slot0 * A.out_per_slot;
                    J.valid = 1; J.code_rate = code_rate;
                    A.jobs[(size_t)list * A.nrows + idx] = J;
                }
            }
        }
        nfr++;
        origin = 14 * (call + 1);
    }
    if constexpr (STREAM) {
        // the capture's latest resume point: the copy in front of a detection, the end of carrier sense, or the origin behind the last event
        if (!fin && !saved) fin_pos = origin;
        if (saved) fin_pos = sv_pos;
        if (n20 != 0) {                                                      // (a zero-length capture leaves its stream as it was)
            const RingLds* src = saved ? SV : reinterpret_cast<const RingLds*>(&W);
            wave_lds_sync();
            uint32_t* rw = rec + 64;
            rw[lane] = src->his[lane >> 5][lane & 31]; rw[64 + lane] = (uint32_t)src->hcr[lane >> 5][lane & 31];
            rw[128 + lane] = (uint32_t)src->hci[lane >> 5][lane & 31]; rw[192 + lane] = (uint32_t)src->he[lane >> 5][lane & 31];
            reinterpret_cast<long long*>(rec + 64 + 256)[lane] = src->his_e[lane];
            const int hw[13] = { (int)kRec11nMagic, saved ? sv_ring : ring_pos, saved ? sv_hisi : his_index, saved ? sv_sr[0] : sr[0], saved ? sv_sr[1] : sr[1],
                                 saved ? sv_si[0] : si[0], saved ? sv_si[1] : si[1], saved ? sv_se[0] : se[0], saved ? sv_se[1] : se[1],
                                 saved ? sv_pf : ld_pf, saved ? sv_pc : ld_pc, saved ? sv_sense : ld_sense, saved ? sv_to : ld_to };
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 13; k++) v = lane == k ? (uint32_t)hw[k] : v;
            rec[lane] = v;
        }
        if (lane == 0) { consumed[cap] = 2 * fin_pos; A.nframes[cap] = nfr; }
        return;
    }
    if (lane == 0) A.nframes[cap] = nfr;
}

__global__ void __launch_bounds__(256) k_scan11n(Scan11nArgs A) { scan11n_body<false>(A, nullptr); }
// the stream form (sora_rx11n_set_stream_mode): cont = the continuation records [ncaps][kRec11nWords], consumed = each capture's latest
// resume point in 40 MHz samples
__global__ void __launch_bounds__(256) k_scan11n_stream(Scan11nArgs A, uint32_t* cont, uint32_t* consumed) { scan11n_body<false, true>(A, nullptr, cont, consumed); }
// The front end of the 40 MHz HT receiver (sora_ht40_process_captures_dev, k_ht40.hip): carrier sense, L-LTF, L-SIG / HT-SIG on the
// duplicated legacy preamble -> one Ht40Found record per event.
__global__ void __launch_bounds__(256) k_scan_ht40(Scan11nArgs A, Ht40Found* found) { scan11n_body<true>(A, found); }
// its stream form (sora_ht40_set_stream_mode): the records and resume points of k_scan11n_stream (kRec11nWords, 40 MHz samples); a20 and end_sample of the
// Ht40Found records stay relative to the capture, so what follows the scan (k_ht40_plan, the data field's kernels) is the same in both modes
__global__ void __launch_bounds__(256) k_scan_ht40_stream(Scan11nArgs A, Ht40Found* found, uint32_t* cont, uint32_t* consumed) { scan11n_body<true, true>(A, found, cont, consumed); }
// the two forms of a handle in SORA_HT40_GUARD_SIGNALLED (sora_ht40_set_guard): HT-SIG's Short GI bit decides a frame's extent
__global__ void __launch_bounds__(256) k_scan_ht40_gi(Scan11nArgs A, Ht40Found* found) { scan11n_body<true, false, true>(A, found); }
__global__ void __launch_bounds__(256) k_scan_ht40_stream_gi(Scan11nArgs A, Ht40Found* found, uint32_t* cont, uint32_t* consumed) { scan11n_body<true, true, true>(A, found, cont, consumed); }

}  // namespace sora
int sora_internal_scan_ht40(const uint32_t* iq0, const uint32_t* iq1, const sora::CapDesc* d_caps, uint32_t ncaps, uint32_t max_frames, sora::Rx11bRow* d_rows, uint32_t* d_nframes,
                            sora::Ht40Found* d_found, const sora::Tables& T, const uint32_t* sincos, const short* atan, hipStream_t st, uint32_t* d_cont, uint32_t* d_consumed,
                            uint32_t joint, uint32_t guard, uint32_t mcs_max)
{
    using namespace sora;
    Scan11nArgs S{};
    S.iq0 = iq0; S.iq1 = iq1; S.caps = d_caps; S.ncaps = ncaps; S.max_frames = max_frames; S.rows = d_rows; S.nframes = d_nframes; S.T = T; S.sincos = sincos; S.atan = atan;
    S.frames = nullptr; S.jobs = nullptr; S.njobs = nullptr; S.nrows = ncaps * max_frames;
    S.mcs_max = mcs_max; S.soft_per_slot = 0; S.out_per_slot = 0; S.joint = joint; S.guard = guard;    // (the HT40 form: its gate, 14 or 15; it queues no 20 MHz data field)
    if (guard) {
        if (d_cont) hipLaunchKernelGGL(k_scan_ht40_stream_gi, dim3((ncaps + 3) / 4), dim3(256), 0, st, S, d_found, d_cont, d_consumed);
        else hipLaunchKernelGGL(k_scan_ht40_gi, dim3((ncaps + 3) / 4), dim3(256), 0, st, S, d_found);
    }
    else
    if (d_cont) hipLaunchKernelGGL(k_scan_ht40_stream, dim3((ncaps + 3) / 4), dim3(256), 0, st, S, d_found, d_cont, d_consumed);
    else hipLaunchKernelGGL(k_scan_ht40, dim3((ncaps + 3) / 4), dim3(256), 0, st, S, d_found);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SORA_OK : sora_internal_fail(SORA_ERR_HARDWARE_FAILED, d_cont ? "k_scan_ht40_stream" : "k_scan_ht40", (int)e);
}
namespace sora {

__global__ void __launch_bounds__(256) k_frame11n(Frame11nArgs A)
{
    __shared__ FrameLds s_w[4];
    __shared__ uint8_t s_lut[6][256];
    fill_demap_luts(s_lut);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const JobRef jr = locate_job(blockIdx.x * 4 + wv, A.njobs);
    if (!jr.ok) return;
    const N11Frame F = A.frames[(size_t)jr.list * A.nrows + jr.idx];
    FrameLds& W = s_w[wv];
    const CapDesc cd = A.caps[F.cap];
    const uint32_t* iq[2] = { A.iq0 + cd.offset, A.iq1 + cd.offset };
    const uint32_t n20 = cd.nsamples / 2;
    auto fetch = [&](int r, uint32_t i) __attribute__((always_inline)) -> uint32_t { return i < n20 ? iq[r][2 * (size_t)i] : 0u; };
    // the packed-arithmetic FFT<64> of k_frame (dev_arith.h): half the instructions of the unpacked one
    const Fft64TwPk tw = fft64_twiddles_pk(A.T, lane & 15);
    const int cfo = uni(F.cfo);
    const uint32_t l0 = (uint32_t)uni((int)F.l0), mcs = (uint32_t)uni((int)F.mcs), nproc = (uint32_t)uni((int)F.nproc);
    const int nb = (int)nbpsc11n(mcs);
    // TStreamJoin<2, 52 nb> -> TStreamConcat<2, s>, s = max(nb / 2, 1): joined position g = lane + 64 t takes element (g / 2s) s + g % s of stream (g / s) & 1,
    // that is soft[stream][deint11n_index]: the lane's de-interleaver entries (offset into W.soft, ten at most: 624 positions) stay in registers
    const int scat = nb >= 4 ? nb / 2 : 1;
    uint32_t dt[10];
#pragma unroll
    for (int t = 0; t < 10; t++) {
        const int g = lane + 64 * t, iss = (g / scat) & 1, k = g / (2 * scat) * scat + g % scat;
        dt[t] = g < 104 * nb ? (uint32_t)(320 * iss + deint11n_index(nb, iss, k)) : 0xFFFFFFFFu;
    }
    int theta = 0;
    // one symbol at 20 MHz index `pos` (its CP included): TFreqComp_11n (running phase n * CFO - theta, n counted from the L-LTF), two FFTs -> W.y[.][64 * half ..]
    auto symbol_fft = [&](uint32_t pos, uint32_t x0, uint32_t x1, int half) __attribute__((always_inline)) {
        const uint32_t n = pos - l0 + 16 + (uint32_t)lane;
        const cpx cof = unpack(A.sincos[(unsigned)((int)n * cfo - theta) & 0xFFFFu]);
        W.buf[0][lane] = pack(freq_comp11n(unpack(x0), cof)); W.buf[1][lane] = pack(freq_comp11n(unpack(x1), cof));
        wave_lds_sync();
        const int g = lane >> 4, e = lane & 15; pcx x[4];
#pragma unroll
        for (int q = 0; q < 4; q++) x[q] = W.buf[g & 1][e + 16 * q];
        fft64_core_pk(x, W.fft[g], e, tw, wave_lds_sync);                               // bin j at slot bitrev6(j) of W.fft[g]
        if (g < 2) {
#pragma unroll
            for (int q = 0; q < 4; q++) W.y[g][64 * half + e + 16 * q] = W.fft[g][__brev((unsigned)(e + 16 * q)) >> 26];
        }
        wave_lds_sync();
    };
    const uint32_t a_ltf = l0 + 128 + 320;                                   // L-LTF (128), three SIG symbols, HT-STF
    // ---- the two HT-LTF symbols -> TMimoChannelEst (channel_11n.hpp:329-443), as k_mimo_est11n_batch
    symbol_fft(a_ltf, fetch(0, a_ltf + 16 + lane), fetch(1, a_ltf + 16 + lane), 0);
    symbol_fft(a_ltf + 80, fetch(0, a_ltf + 96 + lane), fetch(1, a_ltf + 96 + lane), 1);
    {
        const int k = lane < 32 ? lane : lane - 64;
        const bool negate = !(k >= -28 && k <= 28 && kHtLtf[k + 28] == 1);
        cpx hh[2][2]; uint32_t w[4];
        mimo_est_carrier(unpack(W.y[0][lane]), unpack(W.y[0][lane + 64]), unpack(W.y[1][lane]), unpack(W.y[1][lane + 64]), negate, hh, w);
#pragma unroll
        for (int m = 0; m < 4; m++) W.hinv[m][lane] = w[m];
    }
    wave_lds_sync();
    // ---- the data symbols, in order
    const uint32_t a_data = a_ltf + 160;
    const uint32_t S = 104u * (uint32_t)nb;
    // the frame's soft stream, one byte per value (VitJob::soft_bits = 8), in its own symbol slots
    uint8_t* dst = A.soft + (size_t)F.slot0 * A.soft_per_slot;
    uint32_t nx0 = fetch(0, a_data + 16 + lane), nx1 = fetch(1, a_data + 16 + lane);     // the next symbol's samples are requested one symbol ahead
    for (uint32_t d = 0; d < nproc; d++) {
        const uint32_t pos = a_data + 80 * d;
        const uint32_t x0 = nx0, x1 = nx1;
        if (d + 1 < nproc) { nx0 = fetch(0, pos + 96 + lane); nx1 = fetch(1, pos + 96 + lane); }
        symbol_fft(pos, x0, x1, 0);
        // TMimoChannelComp -> TPilotTrack_11n -> demap -> de-interleave -> stream parser
        const cpx p = unpack(W.y[0][lane]), q = unpack(W.y[1][lane]);
        W.xs[0][lane] = pack(mimo_comp_row(unpack(W.hinv[0][lane]), unpack(W.hinv[1][lane]), p, q));
        W.xs[1][lane] = pack(mimo_comp_row(unpack(W.hinv[2][lane]), unpack(W.hinv[3][lane]), p, q));
        wave_lds_sync();
        {
            const int k = lane & 3, sidx = (lane >> 2) & 1;
            const int pbin = k == 0 ? 64 - 21 : k == 1 ? 64 - 7 : k == 2 ? 7 : 21;
            const cpx v = unpack(W.xs[sidx][pbin]);
            int th = dsp_atan16(A.atan, v.re, v.im);
            th += __shfl_xor(th, 1); th += __shfl_xor(th, 2);
            const int t0 = (int)(short)(uni(__shfl(th, 0)) >> 2), t1 = (int)(short)(uni(__shfl(th, 4)) >> 2);
            theta = (int)(short)(theta + (int)(short)((t0 + t1) >> 1));
        }
        if (lane < 52) {
#pragma unroll
            for (int s = 0; s < 2; s++) demap11n_store(W.soft[s] + nb * lane, s_lut, unpack(W.xs[s][data_bin(lane)]), nb);
        }
        wave_lds_sync();
        {
            const uint8_t* both = W.soft[0];
            uint8_t* o = dst + (size_t)d * S + lane;
#pragma unroll
            for (int t = 0; t < 4; t++) if (dt[t] != 0xFFFFFFFFu) o[64 * t] = both[dt[t]];
            if (nb >= 4) {                                                   // 16-QAM: 416 positions, 64-QAM: 624
#pragma unroll
                for (int t = 4; t < 10; t++) if (dt[t] != 0xFFFFFFFFu) o[64 * t] = both[dt[t]];
            }
        }
        wave_lds_sync();
    }
    for (uint32_t g = nproc * S + lane; g < F.nsoft; g += 64) dst[g] = 0;                     // the zero soft values of a flush at the end of the capture
}

// T11aDesc + TBB11aFrameSink (scramble.hpp:319-349, PHY_11a.hpp:660-692) on the decoded bytes of a queued frame -> MPDU slot, error code, FCS
__global__ void __launch_bounds__(256) k_finish11n(Frame11nArgs A)
{
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_z[6 * 8 * 16];
    __shared__ uint32_t s_bufs[4][1504 / 4 + 2];
    s_crc[threadIdx.x] = A.T.crc[threadIdx.x];
    for (int i = threadIdx.x; i < 6 * 8 * 16; i += 256) s_z[i] = A.T.crcz[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = (int)(threadIdx.x >> 6);
    const JobRef jr = locate_job(blockIdx.x * 4 + wv, A.njobs);
    if (!jr.ok) return;
    const N11Frame F = A.frames[(size_t)jr.list * A.nrows + jr.idx];
    uint32_t fcs;
    const uint32_t verdict = finish_frame(A.T, A.vout + (size_t)F.slot0 * A.out_per_slot, F.ht_len, reinterpret_cast<uint8_t*>(s_bufs[wv]),
                                          A.mpdu + (size_t)F.row * 4096, s_crc, s_z, lane, fcs);
    if (lane == 0) { Rx11bRow& r = A.rows[F.row]; r.crc32 = fcs; r.error_code = verdict; }
}

}  // namespace sora

// ------------------------------------------------------------------------------------------------ host side (C ABI, include/sora_hip.h)
#include <vector>
#include <string.h>
#include <stdlib.h>
#include "host_trellis.h"
using namespace sora;


struct Pipe11n : Call {                  // one call in flight: its stream, ticket and completion state (host_calls.h) and every device array a call writes
    CapDesc* d_caps = nullptr; Rx11bRow* d_rows = nullptr; uint32_t* d_nframes = nullptr; uint8_t* d_mpdu = nullptr;
    N11Frame* d_frames = nullptr; VitJob* d_jobs = nullptr; uint32_t* d_njobs = nullptr; uint8_t* d_soft = nullptr; uint8_t* d_vout = nullptr;
    WinScratch win;                         // the window-parallel trellis's vectors and proof record (on its first use)
    std::vector<sora_capture_desc> h_caps; std::vector<CapDesc> h_desc;
    uint32_t ncaps = 0; bool have_results = false;
    DenseStage dense;                       // sora_rx11n_deliver_async
};
struct sora_rx11n {
    sora_rx_cfg cfg{};
    sora_complex16* d_iq_own[2] = { nullptr, nullptr };
    Tables T{}; const uint32_t* sincos = nullptr; const short* atan = nullptr;
    // trellis kernel (sora_rx11n_set_trellis, host_trellis.h): Lanes64 = k_viterbi11n, Lanes16 = k_viterbi16_11n, Windowed = k_viterbi16w_11n + k_win_redo_11n
    // (round 6: the frame's 192-bit trace-back windows side by side, proven afterwards -- k_vitwin.hip), no value = automatic: window-parallel while the handle holds few
    // frames in flight (one wave-slot per frame leaves the chip idle: a lone capture's 8000-step frame was 0.23 ms of a 0.37 ms call), k_viterbi11n above that
    TrellisChoice trellis;
    uint64_t cap_slots = 0;
    // sora_rx11n_set_mcs_max: the SIG parser's gate and the symbol-slot geometry that goes with it (a handle left at the default allocates what it always did)
    int mcs_max = 10; uint32_t soft_per_slot = kSoftPerSlot, out_per_slot = kOutPerSlot;
    static constexpr int kMaxDepth = 8;
    Pipe11n* pipes[kMaxDepth] = {};
    int depth = 1, cur = 0, next_ticket = 0; bool started = false;
    // sora_rx11n_set_stream_mode: the records belong to the handle, not to a pipeline
    StreamRecords records{kRec11nWords};
};

static void pipe11n_free(Pipe11n* p)
{
    if (!p) return;
    if (p->stream) { (void)hipStreamSynchronize(p->stream); (void)hipStreamDestroy(p->stream); }
    if (p->ev_done) (void)hipEventDestroy(p->ev_done);
    (void)hipFree(p->d_caps); (void)hipFree(p->d_rows); (void)hipFree(p->d_nframes); (void)hipFree(p->d_mpdu);
    (void)hipFree(p->d_frames); (void)hipFree(p->d_jobs); (void)hipFree(p->d_njobs); (void)hipFree(p->d_soft); (void)hipFree(p->d_vout);
    p->win.free();
    sora_internal_dense_free(&p->dense);
    delete p;
}
static void rx11n_free(sora_rx11n_t* rx)
{
    if (!rx) return;
    for (Pipe11n* p : rx->pipes) pipe11n_free(p);
    (void)hipFree(rx->d_iq_own[0]); (void)hipFree(rx->d_iq_own[1]); rx->records.free();
    delete rx;
}
// the soft streams and decoded bytes of one pipeline, in the handle's slot geometry; every byte starts out defined: the decoder reads its soft stream in 12-step
// chunks (the tail of a frame's last chunk is read, never used)
static hipError_t pipe11n_slots(const sora_rx11n_t* rx, hipStream_t st, uint8_t** d_soft, uint8_t** d_vout)
{
    const size_t nsoft = (size_t)rx->cap_slots * rx->soft_per_slot + kSoftSlack, nout = (size_t)rx->cap_slots * rx->out_per_slot + 256;
    hipError_t e = hipMalloc((void**)d_soft, nsoft);
    if (e == hipSuccess) e = hipMalloc((void**)d_vout, nout);
    if (e == hipSuccess) e = hipMemsetAsync(*d_soft, 0, nsoft, st);
    if (e == hipSuccess) e = hipMemsetAsync(*d_vout, 0, nout, st);
    return e;
}
static hipError_t pipe11n_create(sora_rx11n_t* rx, Pipe11n** out, int index = 0)
{
    const sora_rx_cfg* cfg = &rx->cfg;
    const size_t rows = (size_t)cfg->max_captures * cfg->max_frames_per_capture;
    Pipe11n* p = new Pipe11n();
    hipError_t e = sora_internal_stream_create(&p->stream, index);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_caps, sizeof(CapDesc) * cfg->max_captures);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_rows, sizeof(Rx11bRow) * rows);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_nframes, 4 * (size_t)cfg->max_captures);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_mpdu, rows * 4096);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_frames, 3 * sizeof(N11Frame) * rows);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_jobs, 3 * sizeof(VitJob) * rows);
    if (e == hipSuccess) e = hipMalloc((void**)&p->d_njobs, 16);
    if (e == hipSuccess) e = pipe11n_slots(rx, p->stream, &p->d_soft, &p->d_vout);
    if (e == hipSuccess) {
        (void)hipMemsetAsync(p->d_frames, 0, 3 * sizeof(N11Frame) * rows, p->stream); (void)hipMemsetAsync(p->d_jobs, 0, 3 * sizeof(VitJob) * rows, p->stream);
    }
    if (e == hipSuccess) { (void)hipMemsetAsync(p->d_rows, 0, sizeof(Rx11bRow) * rows, p->stream); (void)hipMemsetAsync(p->d_nframes, 0,
            4 * (size_t)cfg->max_captures, p->stream); }
    if (e != hipSuccess) { pipe11n_free(p); return e; }
    *out = p;
    return hipSuccess;
}

int sora_rx11n_create(const sora_rx_cfg* cfg, sora_rx11n_t** out)
{
    { const int rc = check_rx_cfg(cfg, out, 40, "sora_rx11n_create"); if (rc) return rc; }
    sora_rx11n_t* rx = new sora_rx11n();
    rx->cfg = *cfg;
    if (!(sora_internal_tables(cfg->device, &rx->T) == SORA_OK && sora_internal_dsp_tables(&rx->sincos, &rx->atan) == SORA_OK)) { rx11n_free(rx);
        return sora_internal_fail(SORA_ERR_HARDWARE_FAILED, "sora_rx11n_create: tables", 0); }
    // symbol slots: 80 samples at 20 MHz each, + 4 per capture (the decoder's padded last burst and its chunked reads may reach past the last symbol)
    rx->cap_slots = cfg->max_total_samples / 2 / 80 + 4 * (uint64_t)cfg->max_captures + 4;
    if (rx->cap_slots * (uint64_t)rx->soft_per_slot * 2 >= (1ull << 32)) { rx11n_free(rx); return sora_internal_fail(SORA_ERR_CAPACITY,
            "sora_rx11n_create: max_total_samples exceeds the 32-bit slot geometry of one handle (split the batch over several handles)", 0); }
    const hipError_t e = pipe11n_create(rx, &rx->pipes[0]);
    if (e != hipSuccess) { rx11n_free(rx); return sora_internal_fail(SORA_ERR_HARDWARE_FAILED, "sora_rx11n_create: device allocation", (int)e); }
    *out = rx;
    return SORA_OK;
}

void* sora_rx11n_stream(sora_rx11n_t* rx) { return rx ? (void*)rx->pipes[rx->cur]->stream : nullptr; }
void sora_rx11n_destroy(sora_rx11n_t* rx) { if (rx) { (void)hipSetDevice(rx->cfg.device); rx11n_free(rx); } }

int sora_rx11n_set_depth(sora_rx11n_t* rx, int depth)
{
    if (!rx) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_set_depth: null handle", 0);
    const int prev = rx->depth;
    if (depth <= 0) return prev;
    if (depth > sora_rx11n::kMaxDepth) depth = sora_rx11n::kMaxDepth;
    { const int rc = sora_rx11n_synchronize(rx); if (rc) return rc; }
    for (int i = 0; i < depth; i++)
        if (!rx->pipes[i]) { const hipError_t e = pipe11n_create(rx, &rx->pipes[i], i);
            if (e != hipSuccess) return sora_internal_fail(SORA_ERR_HARDWARE_FAILED, "sora_rx11n_set_depth: device allocation", (int)e); }
    // a shrink keeps the most recent call addressable: its pipeline moves into the surviving range (the tickets of the pipelines that
    // fall outside it become stale, as the header says)
    if (rx->cur >= depth) { std::swap(rx->pipes[0], rx->pipes[rx->cur]); rx->cur = 0; }
    rx->depth = depth;
    return prev;
}

int sora_rx11n_set_mcs_max(sora_rx11n_t* rx, int mcs_max)
{
    if (!rx) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_set_mcs_max: null handle", 0);
    const int prev = rx->mcs_max;
    if (mcs_max <= 0) return prev;
    if (mcs_max < 10 || mcs_max > 14) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_set_mcs_max: the gate is 10 (the reference's) .. 14", 0);
    { const int rc = sora_rx11n_synchronize(rx); if (rc) return rc; }
    const bool wide = mcs_max > 10;
    const uint32_t soft_per_slot = wide ? kSoftPerSlot11nWide : (uint32_t)kSoftPerSlot, out_per_slot = wide ? kOutPerSlot11nWide : (uint32_t)kOutPerSlot;
    if (soft_per_slot != rx->soft_per_slot) {
        if (rx->cap_slots * (uint64_t)soft_per_slot * 2 >= (1ull << 32)) return sora_internal_fail(SORA_ERR_CAPACITY,
                "sora_rx11n_set_mcs_max: max_total_samples exceeds the 32-bit slot geometry of one handle at this gate (split the batch over several handles)", 0);
        // the pipelines' slot arrays in the new geometry: all of them made before any is replaced, so that a failure leaves the handle as it was
        const uint32_t old_soft = rx->soft_per_slot, old_out = rx->out_per_slot;
        uint8_t* ns[sora_rx11n::kMaxDepth] = {}; uint8_t* nv[sora_rx11n::kMaxDepth] = {};
        rx->soft_per_slot = soft_per_slot; rx->out_per_slot = out_per_slot;
        hipError_t e = hipSuccess;
        for (int i = 0; i < sora_rx11n::kMaxDepth && e == hipSuccess; i++) if (rx->pipes[i]) e = pipe11n_slots(rx, rx->pipes[i]->stream, &ns[i], &nv[i]);
        if (e != hipSuccess) {
            for (int i = 0; i < sora_rx11n::kMaxDepth; i++) { (void)hipFree(ns[i]); (void)hipFree(nv[i]); }
            rx->soft_per_slot = old_soft; rx->out_per_slot = old_out;
            return sora_internal_fail(SORA_ERR_HARDWARE_FAILED, "sora_rx11n_set_mcs_max: device allocation", (int)e);
        }
        for (int i = 0; i < sora_rx11n::kMaxDepth; i++) if (rx->pipes[i]) {
            (void)hipFree(rx->pipes[i]->d_soft); (void)hipFree(rx->pipes[i]->d_vout);
            rx->pipes[i]->d_soft = ns[i]; rx->pipes[i]->d_vout = nv[i];
        }
    }
    if (rx->records.on) { const int rc = rx->records.zero(rx->cfg.max_captures); if (rc) return rc; }     // every stream starts afresh
    rx->mcs_max = mcs_max;
    return prev;
}

// frame rows in flight (depth x max_captures x max_frames_per_capture) up to which the automatic choice is the window-parallel trellis
constexpr long long kAutoWindowedRows11n = 2048;
static Trellis trellis11n_for(const sora_rx11n_t* rx)
{
    if (rx->trellis) return *rx->trellis;
    const long long rows = (long long)rx->depth * (long long)rx->cfg.max_captures * (long long)rx->cfg.max_frames_per_capture;
    return rows <= kAutoWindowedRows11n ? Trellis::Windowed : Trellis::Lanes64;
}
int sora_rx11n_set_trellis(sora_rx11n_t* rx, int lanes_per_pair)
{
    if (!rx) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_set_trellis: null handle", 0);
    const int old = trellis_abi(rx->trellis);
    if (!trellis_parse(lanes_per_pair, &rx->trellis) && lanes_per_pair > 0) return sora_internal_fail(SORA_ERR_INVALID_PARAM,
            "sora_rx11n_set_trellis: 0 (automatic), 16 or 64 lanes per frame pair, or SORA_TRELLIS_WINDOWED", 0);
    return old;
}
int sora_rx11n_trellis(sora_rx11n_t* rx) { return rx ? trellis_abi(trellis11n_for(rx)) : SORA_ERR_INVALID_PARAM; }
// the window-parallel trellis's proof record since the handle was created (as sora_rx_window_stats)
int sora_rx11n_window_stats(sora_rx11n_t* rx, unsigned long long out[4])
{
    if (!rx || !out) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_window_stats: null argument", 0);
    return win_stats_sum(rx->pipes, sora_rx11n::kMaxDepth, rx->cfg.device, out);
}

int sora_rx11n_deliver_async(sora_rx11n_t* rx, int ticket, sora_frame_result* h_rows, size_t max_rows, uint32_t* h_counts, uint8_t* h_mpdu, size_t mpdu_cap)
{
    Pipe11n* P = rx ? call_find(rx->pipes, rx->depth, ticket) : nullptr;
    if (!P) return call_stale("sora_rx11n_deliver_async");
    HIPCHK(hipSetDevice(rx->cfg.device));
    const int rc = sora_internal_dense_deliver(&P->dense, P->d_rows, P->d_nframes, P->d_caps, nullptr, P->ncaps, rx->cfg.max_frames_per_capture, P->d_mpdu, P->stream,
                                               h_rows, max_rows, h_counts, h_mpdu, mpdu_cap);
    if (rc != SORA_OK) return rc;
    HIPCHK(call_mark_delivered(*P));
    return SORA_OK;
}

int sora_rx11n_synchronize(sora_rx11n_t* rx)
{
    if (!rx) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_synchronize: null handle", 0);
    return calls_synchronize(rx->pipes, sora_rx11n::kMaxDepth, rx->cfg.device);
}

int sora_rx11n_set_stream_mode(sora_rx11n_t* rx, int enable)
{
    if (!rx) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_set_stream_mode: null handle", 0);
    if (enable >= 0) { const int rc = sora_rx11n_synchronize(rx); if (rc) return rc; }
    return rx->records.set(enable, rx->cfg.device, rx->cfg.max_captures);
}
int sora_rx11n_stream_consumed(sora_rx11n_t* rx, int ticket, uint32_t* h_consumed, size_t ncaps)
{
    if (!rx || !h_consumed) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_stream_consumed: null argument", 0);
    return rx->records.consumed("sora_rx11n_stream_consumed", rx->cfg.device, call_find(rx->pipes, rx->depth, ticket), ticket == rx->next_ticket, h_consumed, ncaps);
}
// Tickets are looked up, and calls placed, among the first `depth` pipelines: a depth shrink makes the dropped pipelines' tickets stale
int sora_rx11n_ticket(sora_rx11n_t* rx) { return rx && rx->started ? rx->pipes[rx->cur]->ticket : 0; }
int sora_rx11n_wait(sora_rx11n_t* rx, int ticket)
{
    Pipe11n* p = rx ? call_find(rx->pipes, rx->depth, ticket) : nullptr;
    return p ? call_wait(rx->cfg.device, *p) : call_stale("sora_rx11n_wait");
}

int sora_rx11n_wait_any(sora_rx11n_t* rx, int* ticket)
{
    if (!rx || !ticket) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_wait_any: null argument", 0);
    return calls_wait_any(rx->pipes, rx->depth, rx->cfg.device, ticket, "sora_rx11n", [rx](int t) { return sora_rx11n_wait(rx, t); });
}

int sora_rx11n_process_dev(sora_rx11n_t* rx, const sora_complex16* d_iq0, const sora_complex16* d_iq1, const sora_capture_desc* caps, size_t ncaps)
{
    if (!rx || (ncaps && (!d_iq0 || !d_iq1 || !caps))) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_process_dev: null argument", 0);
    if (ncaps > rx->cfg.max_captures) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_rx11n_process_dev: more captures than max_captures", 0);
    HIPCHK(hipSetDevice(rx->cfg.device));
    // stream mode: this call continues the records the one before it leaves, so calls run one after the other
    if (rx->records.on) for (Pipe11n* p : rx->pipes) if (p) HIPCHK(hipStreamSynchronize(p->stream));
    const int idx = call_next(rx->pipes, rx->depth);                             // consecutive calls rotate over the pipelines; a released one first
    Pipe11n* P = rx->pipes[idx];
    std::vector<CapDesc> h(ncaps);                                               // validated first: a refused call leaves the handle's calls intact
    uint64_t total = 0, slots = 0;
    for (size_t i = 0; i < ncaps; i++) {
        if (caps[i].nsamples % 28 != 0) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "capture length must be a whole number of 28-sample source bursts", 0);
        h[i].offset = caps[i].offset; h[i].nsamples = caps[i].nsamples; h[i].capture_id = caps[i].capture_id;
        h[i].slot_base = (uint32_t)slots; h[i].nslots = caps[i].nsamples / 2 / 80 + 4;
        slots += h[i].nslots; total += caps[i].nsamples;
    }
    if (total > rx->cfg.max_total_samples || slots > rx->cap_slots) return sora_internal_fail(SORA_ERR_CAPACITY,
            "sora_rx11n_process_dev: more samples than max_total_samples", 0);
    HIPCHK(hipStreamSynchronize(P->stream));                                  // the call that used this pipeline `depth` calls ago has finished
    P->h_desc.swap(h);
    P->h_caps.assign(caps, caps + ncaps); P->ncaps = (uint32_t)ncaps; P->have_results = true; P->ticket = ++rx->next_ticket; P->delivered = P->released = false;
    rx->cur = idx; rx->started = true;
    if (ncaps == 0) return SORA_OK;
    HIPCHK(hipMemcpyAsync(P->d_caps, P->h_desc.data(), sizeof(CapDesc) * ncaps, hipMemcpyHostToDevice, P->stream));
    Rx11nArgs A;
    A.iq0 = reinterpret_cast<const uint32_t*>(d_iq0); A.iq1 = reinterpret_cast<const uint32_t*>(d_iq1); A.caps = P->d_caps; A.ncaps = (uint32_t)ncaps;
    A.max_frames = rx->cfg.max_frames_per_capture; A.rows = P->d_rows; A.nframes = P->d_nframes; A.mpdu = P->d_mpdu; A.T = rx->T; A.sincos = rx->sincos; A.atan = rx->atan;
    const uint32_t nrows = (uint32_t)ncaps * rx->cfg.max_frames_per_capture;
    HIPCHK(hipMemsetAsync(P->d_njobs, 0, 16, P->stream));
    Scan11nArgs S;
    S.iq0 = A.iq0; S.iq1 = A.iq1; S.caps = P->d_caps; S.ncaps = (uint32_t)ncaps; S.max_frames = A.max_frames; S.rows = P->d_rows; S.nframes = P->d_nframes;
    S.T = rx->T; S.sincos = rx->sincos; S.atan = rx->atan; S.frames = P->d_frames; S.jobs = P->d_jobs; S.njobs = P->d_njobs; S.nrows = nrows;
    S.mcs_max = (uint32_t)rx->mcs_max; S.soft_per_slot = rx->soft_per_slot; S.out_per_slot = rx->out_per_slot; S.joint = 0; S.guard = 0;
    if (rx->records.on) hipLaunchKernelGGL(k_scan11n_stream, dim3((unsigned)((ncaps + 3) / 4)), dim3(256), 0, P->stream, S, rx->records.d_cont, rx->records.d_consumed);
    else hipLaunchKernelGGL(k_scan11n, dim3((unsigned)((ncaps + 3) / 4)), dim3(256), 0, P->stream, S);
    Frame11nArgs F;
    F.iq0 = A.iq0; F.iq1 = A.iq1; F.caps = P->d_caps; F.frames = P->d_frames; F.njobs = P->d_njobs; F.nrows = nrows; F.T = rx->T; F.sincos = rx->sincos; F.atan = rx->atan;
    F.soft = P->d_soft; F.jobs = P->d_jobs; F.vout = P->d_vout; F.rows = P->d_rows; F.mpdu = P->d_mpdu;
    F.soft_per_slot = rx->soft_per_slot; F.out_per_slot = rx->out_per_slot;
    hipLaunchKernelGGL(k_frame11n, dim3((nrows + 3) / 4), dim3(256), 0, P->stream, F);
    const Trellis trellis = trellis11n_for(rx);
    // (the window-parallel trellis's arrays on its first use: its counters are zeroed in this call's stream, in front of its proof)
    if (trellis == Trellis::Windowed) { const int rc = P->win.ensure((uint64_t)rx->cfg.max_captures * rx->cfg.max_frames_per_capture, P->stream, false); if (rc) return rc; }
    trellis_launch<192>(trellis, trellis_lists(P->d_jobs, P->d_njobs, nrows, nrows), P->d_soft, P->d_vout, P->stream, P->win);
    hipLaunchKernelGGL(k_finish11n, dim3((nrows + 3) / 4), dim3(256), 0, P->stream, F);
    HIPCHK(hipGetLastError());
    return SORA_OK;
}

int sora_rx11n_process(sora_rx11n_t* rx, const sora_complex16* h_iq0, const sora_complex16* h_iq1, size_t nsamples, const sora_capture_desc* caps, size_t ncaps)
{
    if (!rx || (nsamples && (!h_iq0 || !h_iq1))) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_process: null argument", 0);
    if (nsamples > rx->cfg.max_total_samples) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_rx11n_process: more samples than max_total_samples", 0);
    { const int rc = check_caps_in_buffer(caps, ncaps, nsamples); if (rc) return rc; }
    HIPCHK(hipSetDevice(rx->cfg.device));
    // the handle's own sample buffers are shared by its pipelines: calls in flight read them
    for (Pipe11n* p : rx->pipes) if (p) HIPCHK(hipStreamSynchronize(p->stream));
    const sora_complex16* src[2] = { h_iq0, h_iq1 };
    for (int k = 0; k < 2; k++) {
        if (!rx->d_iq_own[k]) HIPCHK(hipMalloc((void**)&rx->d_iq_own[k], sizeof(sora_complex16) * (rx->cfg.max_total_samples + 64)));
        HIPCHK(hipMemcpy(rx->d_iq_own[k], src[k], sizeof(sora_complex16) * nsamples, hipMemcpyHostToDevice));
    }
    return sora_rx11n_process_dev(rx, rx->d_iq_own[0], rx->d_iq_own[1], caps, ncaps);
}

int sora_rx11n_results(sora_rx11n_t* rx, sora_frame_result* out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap)
{
    if (!rx || !nout) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_results: null argument", 0);
    *nout = 0;
    const Pipe11n* P = rx->pipes[rx->cur];
    if (!P->have_results) return sora_internal_fail(SORA_ERR_FAILED, "no process call to report", 0);
    return sora_internal_rows_results(P->d_rows, P->d_nframes, P->d_mpdu, P->h_caps.data(), P->ncaps, rx->cfg.max_frames_per_capture, rx->cfg.device, P->stream,
                                      "sora_rx11n_results", out, max_out, nout, h_mpdu, mpdu_cap);
}

int sora_rx11n_results_of(sora_rx11n_t* rx, int ticket, sora_frame_result* out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap)
{
    if (!rx || !nout) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_rx11n_results_of: null argument", 0);
    *nout = 0;
    const Pipe11n* P = call_find(rx->pipes, rx->depth, ticket);
    if (!P) return call_stale("sora_rx11n_results_of");
    return sora_internal_rows_results(P->d_rows, P->d_nframes, P->d_mpdu, P->h_caps.data(), P->ncaps, rx->cfg.max_frames_per_capture, rx->cfg.device, P->stream,
                                      "sora_rx11n_results_of", out, max_out, nout, h_mpdu, mpdu_cap);
}
