// k_tx11n.hip -- 802.11n 2x2 transmitter on the GPU (MCS 8..14, 20 MHz, long GI): the reference's three modulation graphs as
// Test11N_FB_Mod drives them (kernel/bb/demod11/fb11nmod_config.hpp, fb11n_mod.cpp:28-70), one frame after the other:
//   preamble  LSrc / HTSrc (preamble11n.hpp): L-STF, L-LTF | HT-STF, HT-LTF1, HT-LTF2 -- a table built once per device on the host
//   SIG       TBB11nSigSrc -> TConvEncode_12 -> T11aInterleaveBPSK -> TSigMap11n (L-SIG on I, HT-SIG on Q) -> T11aAddPilot<30339>
//             -> TIFFTxOnly -> chain 0 TAddGI, chain 1 TCSD<2> + TAddGI
//   data      TBB11nSrc -> T11aSc -> TBB11nMRSelect -> TConvEncode_{12,23,34} -> TStreamParser*_12 -> T11nInterleave*_S1/_S2
//             -> TMap11a* (30339 / 21453 / 9594 / 4681) -> T11nAddPilot<0/1> -> TIFFTxOnly -> chain 1 TCSD<4> -> TAddGI
// Output: two COMPLEX16 streams at 40 MHz, GetSinkSampleCount() samples each.  Every stage restated as an index map:
//   * FCS, scrambler, encoder, puncturing, mapper, SIG stream, IFFT and emission: dev_tx.h's pieces; the encoder over nvalid input bits --
//     coded bits past its last group are the stream parser's zero padding (tx11n_plan in kernels.h)
//   * stream parser (_b_stream_parser.h): coded bit kc of a symbol goes to stream (kc / s) & 1 as stream bit (kc / 2s) s + kc % s,
//     s = max(1, N_BPSC / 2)
//   * interleaver (interleave.hpp:18-58): stream bit k -> position deint11n_index(N_BPSC, iss, k), the receiver's map; inverted in LDS
//   * mapper: position c N_BPSC + h M + m is bit m (MSB first) of component h (I, Q) of data carrier c (InitQamMapLut), Gray coded
//   * TIFFTxOnly (fft.hpp:63-105): bins 0..31 -> 0..31, 32..63 -> 96..127 of IFFT<128>, no shift; GI = the last 32 of 128
//   * TCSD<n> (csd.hpp): a circular delay of 4 n samples within the 128 before the GI is added
// One 256-thread block per frame.  Eight 32-lane groups: group g carries spatial stream g & 1 of data symbol 4 p + g / 2 in pass p,
// so a group keeps its stream (and its per-lane bit addresses) for the whole frame and a wave's two groups share their symbol.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_tx.h"
#include "dev_11n.h"

namespace sora {

namespace {
constexpr int kWords = 1056;                // generator words per stream: nsym * NDBPS input bits of a 4092-byte MPDU is at most 33696 (MCS 14)
}  // namespace                             // (kBpsk11n, kmod11n, the parser's index rule and the 11n pilots: dev_tx.h)

__global__ void __launch_bounds__(256) k_tx11n(Tx11nArgs A)
{
    __shared__ alignas(16) uint8_t s_data[kWords * 4];
    // generator outputs A (133) / B (171) of the data field, bit i of the stream = bit i & 31 of word i >> 5; zero from nvalid on
    __shared__ uint32_t s_gab[2][kWords];
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_z[6 * 8 * 16];
    __shared__ uint32_t s_bins[8][128];
    __shared__ uint16_t s_inv[2][312];                                           // per stream: interleaved position -> stream bit
    __shared__ uint8_t s_sinv[48];                                               // the SIG symbols' T11aInterleaveBPSK inverted
    __shared__ uint32_t s_crcw[2];
    const uint32_t f = blockIdx.x;
    const int tid = threadIdx.x, g = tid >> 5, e = tid & 31;
    const Tables& T = A.T;
    const uint32_t L = A.len[f];
    Tx11nPlan P;
    if (!tx11n_plan(L, A.mcs[f], P)) return;                                     // an unsupported frame: nothing is written
    const int nb = P.nb, nd = P.ndbps;
    const uint8_t* mp = A.mpdu + A.off[f];
    uint32_t* const out0 = A.out0 + A.out_off[f];
    uint32_t* const out1 = A.out1 + A.out_off[f];
    const uint32_t nsym = P.nsym;
    const uint32_t nw = (nsym * (uint32_t)nd + 31) / 32;                         // generator words the data symbols read

    s_crc[tid] = T.crc[tid];
    for (int i = tid; i < 6 * 8 * 16; i += 256) s_z[i] = T.crcz[i];
    // TBB11nSrc: SERVICE(2) + MPDU + FCS(4) + tail(1) + pad, zero beyond (the encoder's group padding and what the last symbols read)
    for (uint32_t i = tid; i < 4 * nw + 4; i += 256) s_data[i] = (i >= 2 && i < 2 + L) ? mp[i - 2] : (uint8_t)0;
    __syncthreads();
    if (tid < 128) tx_fcs_waves<2>(s_data + 2, L, s_crc, s_z, tid, s_crcw);     // FCS (CF_11nTxVector::crc32 = CalcCRC32 of the MPDU): two waves
    __syncthreads();
    if (tid == 0) {
        const uint32_t fcs = tx_fcs_join<2>(s_z, s_crcw);
        for (int k = 0; k < 4; k++) s_data[2 + L + k] = (uint8_t)(fcs >> (8 * k));
    }
    __syncthreads();
    // T11aSc with DO_SCRAMBLE, TAIL_SCRAMBLE on the tail byte; the register holds the previous 8 output bits
    tx_scramble(s_data, P.nbytes, 2 + L + 4, T.scr_phase[(A.seed ? A.seed[f] : 0xABu) >> 1], T, tid);
    tx_copy_fixed_fields(A.preamble, out0, out1, tid);                           // LSrc, HTSrc
    __syncthreads();
    // TConvEncode_* over the nvalid input bits that exist
    for (uint32_t w = tid; w < nw; w += 256) {
        const uint32_t keep = 32 * w + 32 <= P.nvalid ? 0xFFFFFFFFu : (32 * w >= P.nvalid ? 0u : (1u << (P.nvalid - 32 * w)) - 1u);
        tx_encode_word(reinterpret_cast<const uint32_t*>(s_data), w, keep, s_gab[0][w], s_gab[1][w]);
    }
    for (int k = tid; k < 52 * nb; k += 256) {
        s_inv[0][deint11n_index(nb, 0, k)] = (uint16_t)k;
        s_inv[1][deint11n_index(nb, 1, k)] = (uint16_t)k;
    }
    if (tid < 48) s_sinv[T.deint[tid]] = (uint8_t)tid;                           // T.deint[0..47]: the 11a BPSK interleaver, coded bit -> position
    const Fft128Tw tw = fft128_twiddles(T, e);
    __syncthreads();

    // L-SIG + HT-SIG: 72 bits, rate 1/2 from state 0, three BPSK symbols of 48 coded bits
    if (g < 2 * 2) {                                                             // waves 0 and 1: groups 0..2 carry the three symbols
        // L-SIG LENGTH: the one that spans the HT frame's symbols; HT-SIG: MCS, CBW 20, LENGTH, smoothing, not sounding
        const TxSig72 sig = tx_sig72(((P.nstd + 5) * 24 - 16 - 6) / 8, (A.mcs[f] & 0x7Fu) | (((L + 4) & 0xFFFFu) << 8) | (3u << 24));
        const int s = g;
        uint32_t* const bins = s_bins[g];
        for (int i = e; i < 128; i += 32) bins[i] = 0;
        if (s < 3) {
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int c = e + 32 * t;
                if (c < 48) {
                    const int a = tx_sig_coded_bit(sig, 48 * s + s_sinv[c]) ? kBpsk11n : -kBpsk11n;
                    bins[bin128(carrier_bin48(c))] = s == 0 ? pack(mk(a, 0)) : pack(mk(0, a));   // TSigMap11n: L-SIG on I, HT-SIG on Q
                }
            }
            if (e < 4) tx_put_pilots11a(bins, e, pilot_sgn(s == 0 ? 127u : (unsigned)(s - 1)) ? -kBpsk11n : kBpsk11n);   // m_PilotIndex 127, 0, 1
        }
        tx_ifft128<false>(bins, e, tw);
        if (s < 3) { tx_emit160<false>(bins, e, out0 + 640 + 160 * s, 0); tx_emit160<false>(bins, e, out1 + 640 + 160 * s, 8); }   // chain 1: TCSD<2>
        wave_lds_sync();
    }

    // data symbols.  Per lane, for its stream: up to four components q = e + 32 t (carrier q >> 1, I or Q; carrier q for BPSK), each of
    // M bits at interleaved positions c N_BPSC + h M + m; position -> stream bit -> coded bit kc of the symbol -> (input bit il, generator):
    // symbol-independent (a symbol is a whole number of puncturing periods), held as bit offsets into s_gab.
    const int iss = g & 1;
    const int M = nb == 1 ? 1 : nb / 2, S = M;                                   // S: the stream parser's bits per stream and turn, max(1, N_BPSC / 2)
    const int ncomp = nb == 1 ? 52 : 104;
    uint32_t boff[4][3], cw[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int q = e + 32 * t;
        const int c = nb == 1 ? q : q >> 1, h = nb == 1 ? 0 : q & 1;
        cw[t] = (uint32_t)(q < ncomp ? 4 * bin128(data_bin(c)) + 2 * h : 0);     // byte address of the component's half in the symbol's bins
#pragma unroll
        for (int m = 0; m < 3; m++) {
            boff[t][m] = 0;
            if (q < ncomp && m < M) {
                const int k = s_inv[iss][c * nb + h * M + m];
                const int kc = tx_parse11n_index(S, iss, k);
                boff[t][m] = tx_punct_offset(P.cr, kc, kWords * 32u);
            }
        }
    }
    const int kmod = kmod11n(nb), lvl0 = -((1 << M) - 1) * kmod, kmod2 = 2 * kmod;
    const uint32_t* const gab = &s_gab[0][0];
    uint32_t* const bins = s_bins[g];
    char* const binb = reinterpret_cast<char*>(bins);
    for (uint32_t s0 = 0; s0 < nsym; s0 += 4) {
        const uint32_t s = s0 + (uint32_t)(g >> 1);
        const bool active = s < nsym;
        for (int i = e; i < 128; i += 32) bins[i] = 0;
        if (active) {
            const uint32_t ibase = s * (uint32_t)nd;
            if (nb == 1) {
#pragma unroll
                for (int t = 0; t < 2; t++)
                    if (e + 32 * t < 52) *reinterpret_cast<uint32_t*>(binb + cw[t]) = pack(mk(tx_gen_bit(gab, ibase + boff[t][0]) ? kBpsk11n : -kBpsk11n, 0));
            } else {
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (e + 32 * t < 104) *reinterpret_cast<uint16_t*>(binb + cw[t]) = (uint16_t)tx_axis_level(gab, ibase, boff[t], M, kmod2, lvl0);
                }
            }
            if (e < 4) {
                bins[bin128(pilot_carrier(e) & 63)] = pack(mk(tx_pilot11n(iss, s, e), 0));   // T11nAddPilot<iss>: pilot e of symbol s
            }
        }
        tx_ifft128<false>(bins, e, tw);                                          // (a group past the last symbol only keeps the barriers company)
        if (active) tx_emit160<false>(bins, e, (iss ? out1 : out0) + 1600 + 160 * (size_t)s, iss ? 16 : 0);   // chain 1: TCSD<4>
        wave_lds_sync();
    }
}

}  // namespace sora
