// k_tx_ht40.hip -- 802.11n HT-mixed 40 MHz two-stream transmitter on the GPU (MCS 8..14, long GI): the frame the 40 MHz receiver
// (k_ht40.hip, sora_ht40_*) takes.  PARITY UNPINNED, as for that receiver: the reference has no 40 MHz graph.  The format is the one
// oracle/py_ht40.py::tx_frame defines in float64; the waveform is that frame restated in integers (tests/tx_ht40_model.py), which this
// kernel equals sample for sample:
//   * every frequency-domain value, in units of an HT-LTF carrier, times A = 16384 and rounded: LTF and SIG carriers +-A, both STFs
//     rint(A sqrt(13/12)) = 17053 on I and Q, data levels 6144 / 6144 / 4000 / 2214 (N_BPSC 1 / 2 / 4 / 6) times the Gray map's odd
//     integers, data pilots 12288 on both streams;
//   * every symbol, the training fields included, through the reference's fixed-point IFFT<128> (ifft128_core_pk), GI = the last 32;
//   * L-STF, L-LTF, L-SIG, HT-SIG and HT-STF are the 20 MHz legacy spectrum on both halves of the channel (carrier k at bins k - 32 and,
//     times j, k + 32), identical on both chains, no cyclic shifts; HT-LTFs with P = [[1, -1], [1, 1]]; each spatial stream has its
//     own scrambler seed, K = 7 encoder, puncturing and HT interleaver (N_COL 18, N_ROW 6 N_BPSC, N_ROT 29) and goes out on its own chain.
// Frame: L-STF 320, L-LTF 320, L-SIG 160, HT-SIG 2 x 160, HT-STF 160, HT-LTF 2 x 160, data nsym x 160 samples per chain (short guard interval, k_tx_ht40_gi: nsym x 144).
// One 256-thread block per frame: both streams' scrambled fields and generator words in LDS; eight 32-lane groups, group g carries
// stream g & 1 of data symbol 4 p + g / 2 in pass p.  FCS, scrambler, encoder, puncturing, mapper, SIG stream, IFFT and emission are dev_tx.h's pieces.
// LDS layout: the symbol buffers are swizzled (fft128_swz, dev_arith.h) so that no stage of the IFFT, the 16-byte terminal stage and the
// emission included, meets a bank conflict; a stream's B generator words lie 16 banks from its A words (kGen = 16 mod 32), so the at most
// 17 + 17 consecutive words a symbol's bit gather reads overlap in at most one bank.
//
// The JOINT coding (k_tx_ht40_joint, sora_hip_tx_ht40_joint) is the same frame with ONE PSDU: one field (SERVICE + PSDU + tail + pad up to
// N_SYM x N_DBPS bits, N_DBPS = 2 x 108 N_BPSC R), one FCS, one scrambler pass (one seed, default 0x5D), one K = 7 encoder and puncturing, then the reference's stream
// parser (k_tx11n.hip: with s = max(1, N_BPSC / 2), coded bit kc of a symbol goes to stream (kc / s) & 1 as that stream's bit (kc / 2s) s + kc % s); from there each
// stream's interleaver, mapper and carrier plan are the ones above.  In the kernel the parser is composed with the stream's inverse interleaver in s_inv, so the
// symbol loop is the per-stream one reading one pair of generator-word arrays.  LDS: the field reaches 32832 bits (MCS 13, LENGTH 4000) = 1026 generator words per
// output -- inside one stream's kGen = 1040 -- and 4108 field bytes, more than one stream's kBytes: the two streams' byte arrays are used as one.
#include "dev_tx_ht40.h"

namespace sora {

// The fixed fields, [2 chains][1120]: L-STF 320, L-LTF 320, then HT-STF, HT-LTF1, HT-LTF2 of 160 each -- four transforms of integer bins
// (the short symbol, the long symbol, the HT-LTF and the negated HT-LTF: the fixed-point transform of -X is not minus that of X), one per
// 32-lane group.  One block of 128 threads.
__global__ void __launch_bounds__(128) k_tx_ht40_preamble(uint32_t* tab, Tables T)
{
    __shared__ alignas(16) uint32_t s_bins[4][128];
    const int tid = threadIdx.x, g = tid >> 5, e = tid & 31;
    uint32_t* const bins = s_bins[g];
    for (int i = e; i < 128; i += 32) bins[i] = 0;
    if (g == 0) {
        if (e < 13) { const int v = kLStf[e] * kStf; put_dup40(bins, 4 * e - 24, v, v); }
    } else if (g == 1) {
        for (int i = e; i < 53; i += 32) put_dup40(bins, i - 26, kLLtf[i] * kAmp, 0);
    } else {
        for (int i = e; i < 117; i += 32) bins[fft128_swz((i - 58) & 127)] = pk16((g == 2 ? kAmp : -kAmp) * kHtLtf40[i], 0);
    }
    tx_ifft128<true>(bins, e, fft128_twiddles(T, e));
    uint32_t* const t0 = tab, * const t1 = tab + kTxHt40Preamble;
    if (g == 0) {
        for (int i = e; i < 320; i += 32) t0[i] = t1[i] = tx_tsample<true>(bins, (uint32_t)i);                        // the symbol tiled
        for (int i = e; i < 160; i += 32) t0[640 + i] = t1[640 + i] = tx_tsample<true>(bins, (uint32_t)i);
    } else if (g == 1) {
        for (int i = e; i < 320; i += 32) t0[320 + i] = t1[320 + i] = tx_tsample<true>(bins, (uint32_t)(i + 64));     // GI2 of 64, two symbols
    } else if (g == 2) {
        for (int i = e; i < 160; i += 32) t0[800 + i] = t1[800 + i] = t1[960 + i] = tx_tsample<true>(bins, (uint32_t)(i + 96));
    } else {
        for (int i = e; i < 160; i += 32) t0[960 + i] = tx_tsample<true>(bins, (uint32_t)(i + 96));                  // P = [[1, -1], [1, 1]]
    }
}

__global__ void __launch_bounds__(256) k_tx_ht40(TxHt40Args A) { tx_ht40_body<false>(A); }
__global__ void __launch_bounds__(256) k_tx_ht40_joint(TxHt40Args A) { tx_ht40_body<true>(A); }
__global__ void __launch_bounds__(256) k_tx_ht40_gi(TxHt40Args A) { tx_ht40_body<false, true>(A); }
__global__ void __launch_bounds__(256) k_tx_ht40_joint_gi(TxHt40Args A) { tx_ht40_body<true, true>(A); }

}  // namespace sora
