// dev_tx_ht40.h -- the body of the 40 MHz HT 2x2 transmitter's kernels (k_tx_ht40.hip describes the frame and the LDS plan) and the constants and helpers it shares with
// k_tx_ht40_preamble, stated once for the two files that instantiate it: k_tx_ht40.hip (k_tx_ht40, _joint, _gi, _joint_gi) and k_tx_ht40_mcs.hip (k_tx_ht40_mcs,
// k_tx_ht40_joint_mcs: the gate at 15).  Two files, so that the first one's kernels are compiled among the same functions as before MCS 15 existed.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_tx.h"
#include "dev_ht40.h"

namespace sora {

namespace {
constexpr int kBytes = 4096;                // field bytes per stream: SERVICE + 3996 + FCS + tail, up to the last generator word read (4068)
constexpr int kGen = 1040;                  // generator words per stream and output: nsym * NDBPS input bits are at most 32507 (1016 words)
constexpr int kAmp = kTxHt40Amp;            // A: an LTF / SIG carrier
constexpr int kStf = 17053;                 // rint(A sqrt(13 / 12))
static_assert(kGen % 32 == 16 && kGen * 32 >= 32507 && kBytes >= 4 * 1016 + 4, "LDS plan");
static_assert(kGen >= 1026 && 2 * kBytes >= 4 * 1026 + 4, "LDS plan, joint coding: 32832 field bits = 1026 generator words, 4108 field bytes in the two streams' arrays");
// MCS 15 (N_DBPS 540 per stream, 1080 joint): a field is at most 8 x 4000 + 22 bits rounded up to a whole symbol, below 32022 + 539 = 32561 bits per stream (1018 words,
// 4076 bytes) and 32022 + 1079 = 33101 joint (1035 words, 4144 bytes in the two streams' arrays)
static_assert(kGen * 32 >= 33101 && kGen >= 1035 && kBytes >= 4 * 1018 + 4 && 2 * kBytes >= 4 * 1035 + 4, "LDS plan, MCS 15");
__device__ __forceinline__ uint32_t pk16(int re, int im) { return (uint32_t)(uint16_t)re | ((uint32_t)(uint16_t)im << 16); }
static __constant__ int8_t kLLtf[53] = {    // L-LTF, carriers -26..26
    1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 0,
    1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1 };
static __constant__ int8_t kLStf[13] = { 1, -1, 1, -1, -1, 1, 0, -1, -1, 1, 1, 1, 1 };   // x (1 + j), carriers -24, -20, .., 24
// data carrier c (0..47) of a legacy symbol: -26..26 without 0, +-7, +-21
__device__ __forceinline__ int leg_carrier(int c) { const int b = carrier_bin48(c); return b < 32 ? b : b - 64; }
// legacy carrier k with value (re, im) on both halves of the channel: bin k - 32 as it is, bin k + 32 times j
__device__ __forceinline__ void put_dup40(uint32_t* bins, int k, int re, int im)
{
    bins[fft128_swz((k - 32) & 127)] = pk16(re, im);
    bins[fft128_swz((k + 32) & 127)] = pk16(-im, re);
}
}  // namespace

// GI = true (k_tx_ht40_gi, k_tx_ht40_joint_gi; sora_hip_tx_ht40_gi): the frame's guard-interval kind A.gi[f] is read once, is block-uniform and
// selects the data symbols' pitch and emission (160 / tx_emit160 or 144 / tx_emit144), HT-SIG bit 31 and the L-SIG length; a kind other than 0 / 1 is a frame that is not
// accepted.  Every addition sits under "if constexpr (GI)": the kernels without it are the instruction streams they were.
// M15 = true (k_tx_ht40_mcs, k_tx_ht40_joint_mcs; sora_hip_tx_ht40_mcs with the gate at 15): MCS 15 is accepted too -- the gated plan, and the
// puncture map that knows rate 5/6; HT-SIG carries the MCS as it is.  Both additions sit under "if constexpr (M15)".
template <bool JOINT, bool GI = false, bool M15 = false>
__device__ __forceinline__ void tx_ht40_body(const TxHt40Args& A)
{
    __shared__ alignas(16) uint8_t s_data[2][kBytes];
    // generator outputs A (133) / B (171) of each stream's data field, bit i of the stream = bit i & 31 of word i >> 5
    __shared__ uint32_t s_gab[2][2][kGen];
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_z[6 * 8 * 16];
    __shared__ alignas(16) uint32_t s_bins[8][128];
    __shared__ uint16_t s_inv[2][648];                                           // per stream: interleaved position -> coded bit of the symbol
    __shared__ uint32_t s_crcw[4];
    const uint32_t f = blockIdx.x;
    const int tid = threadIdx.x, g = tid >> 5, e = tid & 31;
    const Tables& T = A.T;
    const uint32_t L = A.len[f], mcs = A.mcs[f];
    TxHt40Plan P;
    if constexpr (M15) { if (!tx_ht40_plan_mcs(L, mcs, 15u, JOINT, P)) return; }
    else
    if (!(JOINT ? tx_ht40_plan_joint(L, mcs, P) : tx_ht40_plan(L, mcs, P))) return;   // a frame that is not accepted: nothing is written
    [[maybe_unused]] uint32_t sgi = 0;
    if constexpr (GI) { sgi = A.gi ? (uint32_t)A.gi[f] : 0u; if (sgi > 1u) return; }
    const int nb = P.nb, nd = P.ndbps;
    const uint32_t nsym = P.nsym;
    const uint32_t nw = (nsym * (uint32_t)nd + 31) / 32;                         // generator words the data symbols read, per stream (joint: of the one field)
    [[maybe_unused]] uint8_t* const jdata = &s_data[0][0];                       // joint: the one field, over both streams' byte arrays
    uint32_t* const out0 = A.out0 + A.out_off[f];
    uint32_t* const out1 = A.out1 + A.out_off[f];

    s_crc[tid] = T.crc[tid];
    for (int i = tid; i < 6 * 8 * 16; i += 256) s_z[i] = T.crcz[i];
    // per stream: SERVICE(2) + MPDU + FCS(4) + tail + pad, zero beyond
    if constexpr (JOINT) {
        const uint8_t* mp = A.mpdu + A.off[f];
        for (uint32_t i = tid; i < 4 * nw + 4; i += 256) jdata[i] = (i >= 2 && i < 2 + L) ? mp[i - 2] : (uint8_t)0;
    }
    else
#pragma unroll
    for (int st = 0; st < 2; st++) {
        const uint8_t* mp = A.mpdu + A.off[2 * f + st];
        for (uint32_t i = tid; i < 4 * nw + 4; i += 256) s_data[st][i] = (i >= 2 && i < 2 + L) ? mp[i - 2] : (uint8_t)0;
    }
    __syncthreads();
    // FCS of both MPDUs: stream tid >> 7, two waves each
    if constexpr (JOINT) { if (tid < 128) tx_fcs_waves<2>(jdata + 2, L, s_crc, s_z, tid, s_crcw); }
    else
    tx_fcs_waves<2>(s_data[tid >> 7] + 2, L, s_crc, s_z, tid & 127, s_crcw + 2 * (tid >> 7));
    __syncthreads();
    if constexpr (JOINT) {
        if (tid == 0) {
            const uint32_t fcs = tx_fcs_join<2>(s_z, s_crcw);
            for (int k = 0; k < 4; k++) jdata[2 + L + k] = (uint8_t)(fcs >> (8 * k));
        }
    }
    else
    if (tid < 2) {
        const uint32_t fcs = tx_fcs_join<2>(s_z, s_crcw + 2 * tid);
        for (int k = 0; k < 4; k++) s_data[tid][2 + L + k] = (uint8_t)(fcs >> (8 * k));
    }
    __syncthreads();
    // scrambler: x[n] = x[n-4] ^ x[n-7], seed bit i = x[-1-i] (py_ht40.scramble_seq); the phase tables keep the register the other way
    // round.  Everything up to the last symbol's last bit is scrambled, pad included; the six tail bits are forced to zero afterwards.
    if constexpr (JOINT) {
        const unsigned seed = A.seed ? A.seed[f] : 0x5Du;
        tx_scramble(jdata, (nsym * (uint32_t)nd + 7) / 8, 2 + L + 4, T.scr_phase[brev7(seed & 0x7Fu)], T, tid);
    }
    else
#pragma unroll
    for (int st = 0; st < 2; st++) {
        const unsigned seed = A.seed ? A.seed[2 * f + st] : (st ? 0x2Bu : 0x5Du);
        tx_scramble(s_data[st], (nsym * (uint32_t)nd + 7) / 8, 2 + L + 4, T.scr_phase[brev7(seed & 0x7Fu)], T, tid);
    }
    tx_copy_fixed_fields(A.preamble, out0, out1, tid);
    __syncthreads();
    // the K = 7 encoder, each stream's field on its own (joint: the one field into stream 0's generator words)
    if constexpr (JOINT) {
        for (uint32_t w = tid; w < nw; w += 256) tx_encode_word(reinterpret_cast<const uint32_t*>(jdata), w, 0xFFFFFFFFu, s_gab[0][0][w], s_gab[0][1][w]);
    }
    else
    for (uint32_t i = tid; i < 2 * nw; i += 256) {
        const int st = i >= nw;
        const uint32_t w = st ? i - nw : i;
        tx_encode_word(reinterpret_cast<const uint32_t*>(s_data[st]), w, 0xFFFFFFFFu, s_gab[st][0][w], s_gab[st][1][w]);
    }
    if constexpr (JOINT) {
        // the stream parser composed with the inverse interleaver: bit k of stream iss is coded bit (k / s) 2s + iss s + k % s of the symbol
        const int sp = nb / 2 > 1 ? nb / 2 : 1;
        for (int k = tid; k < 108 * nb; k += 256) {
            const int kc = (k / sp) * 2 * sp + k % sp;
            s_inv[0][deint40_index(nb, 0, k)] = (uint16_t)kc;
            s_inv[1][deint40_index(nb, 1, k)] = (uint16_t)(kc + sp);
        }
    }
    else
    for (int k = tid; k < 108 * nb; k += 256) {
        s_inv[0][deint40_index(nb, 0, k)] = (uint16_t)k;
        s_inv[1][deint40_index(nb, 1, k)] = (uint16_t)k;
    }
    const Fft128Tw tw = fft128_twiddles(T, e);
    uint32_t* const bins = s_bins[g];
    __syncthreads();

    // L-SIG + HT-SIG: 24 + 48 bits at rate 1/2 from state 0 (L-SIG's six tail bits return the encoder to it), three BPSK symbols of 48 coded
    // bits through the legacy interleaver (coded bit k at position 3 (k mod 16) + k div 16), L-SIG on I, HT-SIG on Q, pilots 1, 1, 1, -1
    if (g < 4) {                                                                 // waves 0 and 1: groups 0..2 carry the three symbols
        // L-SIG LENGTH: the legacy duration that spans the HT frame; HT-SIG: MCS, CBW 40, LENGTH, smoothing, not sounding, reserved
        TxSig72 sig;
        if constexpr (GI) sig = tx_sig72(tx_ht40_lsig_length(nsym, sgi), (mcs & 0x7Fu) | (1u << 7) | (((L + 4) & 0xFFFFu) << 8) | (7u << 24) | (sgi << 31));   // bit 31: Short GI
        else sig = tx_sig72(12u + 3u * nsym, (mcs & 0x7Fu) | (1u << 7) | (((L + 4) & 0xFFFFu) << 8) | (7u << 24));
        const int s = g;
        for (int i = e; i < 128; i += 32) bins[i] = 0;
        if (s < 3) {
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int c = e + 32 * t;
                if (c < 48) {
                    const int a = tx_sig_coded_bit(sig, 48 * s + 16 * (c % 3) + c / 3) ? kAmp : -kAmp;
                    put_dup40(bins, leg_carrier(c), s == 0 ? a : 0, s == 0 ? 0 : a);
                }
            }
            if (e < 4) put_dup40(bins, pilot_carrier(e), e == 3 ? -kAmp : kAmp, 0);
        }
        tx_ifft128<true>(bins, e, tw);
        if (s < 3) { tx_emit160<true>(bins, e, out0 + 640 + 160 * s, 0); tx_emit160<true>(bins, e, out1 + 640 + 160 * s, 0); }   // no cyclic shifts
        wave_lds_sync();
    }

    // data symbols.  Per lane, for its stream: up to four carriers c = e + 32 t, each of M bits per axis at interleaved positions
    // c N_BPSC + h M + m (h: I, Q); position -> coded bit kc of the symbol -> (input bit il, generator): symbol-independent (a symbol is a
    // whole number of puncturing periods), held as bit offsets into the stream's generator words.
    const int iss = g & 1;
    const int M = nb == 1 ? 1 : nb / 2, nax = nb == 1 ? 1 : 2;
    uint32_t boff[4][6], cw[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int c = e + 32 * t;
        cw[t] = (uint32_t)fft128_swz(data_bin40(c < 108 ? c : 0));
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int m = 0; m < 3; m++) {
                boff[t][3 * h + m] = 0;
                if (c < 108 && h < nax && m < M)
                    boff[t][3 * h + m] = M15 ? tx_punct_offset56(P.cr, s_inv[iss][c * nb + h * M + m], kGen * 32u)
                                             : tx_punct_offset(P.cr, s_inv[iss][c * nb + h * M + m], kGen * 32u);
            }
    }
    const int d = level40(nb), lvl0 = -((1 << M) - 1) * d, d2 = 2 * d;
    const uint32_t* const gab = &s_gab[JOINT ? 0 : iss][0][0];
    uint32_t* const out = iss ? out1 : out0;
    for (uint32_t s = (uint32_t)(g >> 1); s < nsym; s += 4) {                    // (a wave's two groups share their symbol: the trip count is the wave's)
        const uint32_t ibase = s * (uint32_t)nd;
        // the 14 bins that carry nothing: 127, 0, 1 and 59..69 (the buffer holds the symbol before's samples)
        if (e < 14) bins[fft128_swz(e < 3 ? (e + 127) & 127 : 56 + e)] = 0;
        if (e < 6) bins[fft128_swz((e == 0 ? -53 : e == 1 ? -25 : e == 2 ? -11 : e == 3 ? 11 : e == 4 ? 25 : 53) & 127)] = pk16(kPilot40, 0);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (e + 32 * t < 108) {
                int ax[2] = { 0, 0 };
                if (nb == 1) ax[0] = tx_gen_bit(gab, ibase + boff[t][0]) ? d : -d;
                else {
#pragma unroll
                    for (int h = 0; h < 2; h++) ax[h] = tx_axis_level(gab, ibase, boff[t] + 3 * h, M, d2, lvl0);
                }
                bins[cw[t]] = pk16(ax[0], ax[1]);
            }
        }
        tx_ifft128<true>(bins, e, tw);
        if constexpr (GI) {
            if (sgi) tx_emit144<true>(bins, e, out + 1600 + kHt40ShortSym * (size_t)s);
            else tx_emit160<true>(bins, e, out + 1600 + 160 * (size_t)s, 0);
        }
        else
        tx_emit160<true>(bins, e, out + 1600 + 160 * (size_t)s, 0);
        wave_lds_sync();
    }
}
}  // namespace sora
