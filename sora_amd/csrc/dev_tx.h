// dev_tx.h -- the pieces of the transmit graphs (fb11amod_config.hpp:74-110, fb11nmod_config.hpp, fb11bmod_config.hpp:28-50), each stated once:
//   TBB11aSrc / TBB11nSrc / TBB11bSrc (FCS) -> T11aSc -> TConvEncode_{12,23,34} -> interleaver -> TMap11a* -> T11aAddPilot -> TIFFTx / TIFFTxOnly -> TAddGI
// k_tx.hip, k_tx11n.hip and k_tx_ht40.hip take the reference's arithmetic from here and keep their own frame geometry, LDS layout, interleaver tables and
// schedule; k_tx11b.hip takes the FCS and nothing else.  Where the kernels differ in a value (a seed's phase, a tail index, a mask, an amplitude, a cyclic
// shift, whether the symbol buffer is swizzled) the value is an argument; no piece asks which kernel calls it.
#pragma once
#include "kernels.h"
#include "dev_pilot11a.h"

namespace sora {

__device__ __forceinline__ uint32_t brev7(uint32_t n) { return __brev(n) >> 25; }                 // FFT128LUTMap: 7-bit bit reversal
__device__ __forceinline__ int bin128(int bin64) { return bin64 < 32 ? bin64 : bin64 + 64; }      // TIFFTx / TIFFTxOnly (fft.hpp:21-105): bins 32..63 of 64 go to 96..127 of IFFT<128>

// ---- FCS of an MPDU (PHY_11a.hpp:87,160-170; CF_11nTxVector::crc32; PHY_11b.hpp: CalcCRC32), by WAVES waves of crc32_wave: lanes l = 0 .. 64 WAVES - 1 call
// tx_fcs_waves, a block barrier follows, then tx_fcs_join is the FCS.  Wave 1 takes the kCrcWaveBytes bytes before the last kCrcWaveBytes:
// CRC(0, M1 | M2) = Z_2560(CRC(0, M1)) ^ CRC(0, M2).  n < 4 (crc32_wave's complement of the first four bytes needs them): lane 0, byte by byte.
constexpr int kCrcWaveBytes = 64 * 40;                                           // what one wave of crc32_wave covers
template <int WAVES>
__device__ __forceinline__ void tx_fcs_waves(const uint8_t* msg, uint32_t n, const uint32_t* s_crc, const uint32_t* s_z, int l, uint32_t* s_crcw)
{
    if (n >= 4) {
        const uint32_t c = crc32_wave(msg, (int)n, s_crc, s_z, l);
        if ((l & 63) == 0) s_crcw[l >> 6] = c;
    } else if (l == 0) {
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < n; i++) c = (c >> 8) ^ s_crc[(msg[i] ^ c) & 0xFF];
        s_crcw[0] = c;
        if (WAVES == 2) s_crcw[1] = 0;
    }
}
template <int WAVES>
__device__ __forceinline__ uint32_t tx_fcs_join(const uint32_t* s_z, const uint32_t* s_crcw)
{
    static_assert(WAVES == 1 || WAVES == 2, "Z_2560 = two steps of crc_zeros level 5 (1280 bytes)");
    return ~(WAVES == 2 ? crc_zeros(s_z, 5, crc_zeros(s_z, 5, s_crcw[1])) ^ s_crcw[0] : s_crcw[0]);
}

// ---- T11aSc (scramble.hpp:233-258): the register sequence is a phase of one period-127 cycle, so byte i takes the eight bits from phase + 8 i on
// (phase = T.scr_phase[register], 255: the all-zero register stays zero); the tail byte keeps only its two pad bits (TAIL_SCRAMBLE).
__device__ __forceinline__ void tx_scramble(uint8_t* field, uint32_t nbytes, uint32_t tail, unsigned phase, const Tables& T, int tid)
{
    for (uint32_t i = tid; i < nbytes; i += 256) {
        unsigned c = field[i] ^ (phase == 255 ? 0u : T.scr_seq[(phase + 8u * i) % 127u]);
        if (i == tail) c &= 0xC0u;
        field[i] = (uint8_t)c;
    }
}

// ---- TConvEncode_* (conv_enc.hpp:6-14) 32 input bits at a time: A = x ^ x>>2 ^ x>>3 ^ x>>5 ^ x>>6 (133), B = x ^ x>>1 ^ x>>2 ^ x>>3 ^ x>>6 (171) over the bit
// stream (x>>k = the bit k positions EARLIER: shifted in from the previous word; the encoder starts from state 0).  keep: the input bits that exist.
__device__ __forceinline__ void tx_encode_word(const uint32_t* dw, uint32_t w, uint32_t keep, uint32_t& ga, uint32_t& gb)
{
    const uint32_t X = dw[w], P = w ? dw[w - 1] : 0u;
    auto sh = [&](int k) { return (X << k) | (P >> (32 - k)); };
    const uint32_t x2 = sh(2), x3 = sh(3), x6 = sh(6);
    ga = (X ^ x2 ^ x3 ^ sh(5) ^ x6) & keep;
    gb = (X ^ sh(1) ^ x2 ^ x3 ^ x6) & keep;
}
// ---- the puncturing patterns (conv_enc.hpp: TConvEncode_12 / _23 / _34) as an index map: coded bit k of a symbol is generator `which` at input bit il of the symbol; returned as the
// bit's offset into generator words laid out A then B, gen_bits apart.  cr: 0 = 1/2, 1 = 2/3, 2 = 3/4.  Does not depend on the symbol: N_CBPS is a whole
// number of puncturing periods.
__device__ __forceinline__ uint32_t tx_punct_offset(int cr, int k, uint32_t gen_bits)
{
    int il, which;
    if (cr == 0) { il = k >> 1; which = k & 1; }
    else if (cr == 1) { const int q3 = k / 3, r = k - 3 * q3; il = 2 * q3 + (r == 2); which = r == 1; }
    else { const int q4 = k >> 2, r = k & 3; il = 3 * q4 + (r == 2 ? 1 : r == 3 ? 2 : 0); which = r & 1; }
    return (uint32_t)il + (uint32_t)which * gen_bits;
}

// ... with rate 5/6 beside them (cr 3, SORA_CR_56: the 40 MHz pair's MCS 15; the reference has no such encoder): A1 B1 A2 B3 A4 B5 -- coded bit k = 6 q + r is generator
// A (r even) or B (r odd) at input bit 5 q + (0, 0, 1, 2, 3, 4)[r].  N_CBPS = 108 N_BPSC per stream is a whole number of these periods too.  A function of its own: what
// calls tx_punct_offset compiles to what it did.
__device__ __forceinline__ uint32_t tx_punct_offset56(int cr, int k, uint32_t gen_bits)
{
    if (cr != 3) return tx_punct_offset(cr, k, gen_bits);
    const int q6 = k / 6, r = k - 6 * q6;
    return (uint32_t)(5 * q6 + (r == 0 ? 0 : r - 1)) + (uint32_t)(r & 1) * gen_bits;
}

// ---- TMap11a* (mapper11a.hpp:16-43): bit idx of the generator words; one axis of a carrier from its M <= 3 bits, first-transmitted = MSB (InitQamMapLut's
// reversal), Gray -> binary, level bb * 2 d + lvl0 with lvl0 = -(2^M - 1) d
__device__ __forceinline__ uint32_t tx_gen_bit(const uint32_t* gab, uint32_t idx) { return (gab[idx >> 5] >> (idx & 31u)) & 1u; }
__device__ __forceinline__ int tx_axis_level(const uint32_t* gab, uint32_t ibase, const uint32_t off[3], int M, int d2, int lvl0)
{
    unsigned v = 0;
#pragma unroll
    for (int m = 0; m < 3; m++) if (m < M) v |= tx_gen_bit(gab, ibase + off[m]) << (M - 1 - m);
    unsigned bb = v ^ (v >> 1); bb ^= bb >> 2;
    return (int)bb * d2 + lvl0;
}

// ---- PLCP SIGNAL / L-SIG (ieee80211a_cmn.h:8-26, _b_lsig.h): RATE, LENGTH, even parity; tail 0
__device__ __forceinline__ uint32_t tx_lsig(uint32_t rate_code, uint32_t length)
{
    const uint32_t sig = rate_code | (length << 5);
    return sig | ((uint32_t)(__popc(sig) & 1) << 17);
}
// ---- L-SIG + HT-SIG (TBB11nSigSrc, _b_lsig.h, _b_htsig.h): 72 bits -- L-SIG at 6 Mbps with the LENGTH that spans the HT frame, then HT-SIG: h4 (its bits
// 0..31: MCS, CBW, LENGTH, the flags), NES 0, CRC bits 34..41 (CalcCRC8(cdata, 4, 2): reflected, poly 0xE0, over 34 bits, complemented), tail 0
struct TxSig72 { uint64_t lo; uint32_t hi; };                                    // bits 0..63, bits 64..71
__device__ __forceinline__ TxSig72 tx_sig72(uint32_t lsig_length, uint32_t h4)
{
    uint32_t crc = 0xFF;
    for (int b = 0; b < 34; b++) { crc ^= b < 32 ? (h4 >> b) & 1u : 0u; crc = (crc & 1u) ? (crc >> 1) ^ 0xE0u : crc >> 1; }
    crc = ~crc & 0xFFu;
    const uint64_t ht = (uint64_t)h4 | ((uint64_t)crc << 34);
    return TxSig72{ (uint64_t)tx_lsig(0xBu, lsig_length) | (ht << 24), (uint32_t)(ht >> 40) };
}
// coded bit kg (0..143) of the three SIG symbols: TConvEncode_12 from state 0 over the 72 bits (L-SIG's six tail bits return the encoder to it)
__device__ __forceinline__ uint32_t tx_sig_coded_bit(const TxSig72& S, int kg)
{
    auto bit = [&](int i) -> uint32_t { return i < 0 ? 0u : i < 64 ? (uint32_t)(S.lo >> i) & 1u : (S.hi >> (i - 64)) & 1u; };
    const int i = kg >> 1;
    return (kg & 1) ? bit(i) ^ bit(i - 1) ^ bit(i - 2) ^ bit(i - 3) ^ bit(i - 6) : bit(i) ^ bit(i - 2) ^ bit(i - 3) ^ bit(i - 5) ^ bit(i - 6);
}

// ---- T11aAddPilot (pilot.hpp:76-118) on the 128-point grid: lane k < 4 puts pilot k of a symbol, p the symbol's polarity times the amplitude
__device__ __forceinline__ void tx_put_pilots11a(uint32_t* bins, int k, int p)
{
    bins[bin128(pilot_carrier(k) & 63)] = pack(mk(k == 3 ? -p : p, 0));
}

// ---- the 802.11n 2x2 data graph (fb11nmod_config.hpp), the pieces k_tx11n.hip and the stages of k_mod11n.hip share
constexpr int kBpsk11n = 30339;             // fb11nmod_config.hpp: TMap11aBPSK<30339>, T11nAddPilot, T11aAddPilot<30339>, TSigMap11n
__device__ __forceinline__ int kmod11n(int nb) { return nb == 1 ? kBpsk11n : nb == 2 ? 21453 : nb == 4 ? 9594 : 4681; }
// TStreamParser*_12 (_b_stream_parser.h): bit k of spatial stream iss is coded bit ((k / S) 2 + iss) S + k % S of the symbol, S = max(1, N_BPSC / 2) bits per stream and turn
__device__ __forceinline__ int tx_parse11n_index(int S, int iss, int k) { return ((k / S) * 2 + iss) * S + k % S; }
// T11nAddPilot<iss> (pilot_11n.hpp:44-73, _b_dot11_pilot.h): pilot k of symbol n = polarity[(n + 3) % 127] x Psi_iss[(n + k) & 3] x 30339,
// Psi_0 = {1, 1, -1, -1}, Psi_1 = {1, -1, -1, 1}; k = 0..3 at carriers -21, -7, 7, 21
__device__ __forceinline__ int tx_pilot11n(int iss, uint32_t n, int k)
{
    const int j = (int)((n + (uint32_t)k) & 3u);
    const int psi = iss == 0 ? (j < 2 ? 1 : -1) : ((j == 0 || j == 3) ? 1 : -1);
    return (pilot_sgn((n + 3u) % 127u) ? -psi : psi) * kBpsk11n;
}

// ---- IFFT<128> of a group's 128-word symbol buffer in place (ifft128_core_pk: packed COMPLEX16, bit-exact with fft128_core<true>): time sample n is left at
// word brev7(n), swizzled (fft128_swz) where the buffer is.  The buffer is private to a 32-lane group: wave-level barriers.
template <bool SWZ>
__device__ __forceinline__ void tx_ifft128(uint32_t* s, int e, const Fft128Tw& tw)
{
    pcx x[4];
    wave_lds_sync();
#pragma unroll
    for (int m = 0; m < 4; m++) x[m] = s[SWZ ? fft128_swz(e + 32 * m) : e + 32 * m];
    ifft128_core_pk<SWZ>(x, s, e, tw, wave_lds_sync);
}
template <bool SWZ>
__device__ __forceinline__ uint32_t tx_tsample(const uint32_t* s, uint32_t n) { const int w = (int)brev7(n & 127u); return s[SWZ ? fft128_swz(w) : w]; }
// ---- TCSD<csd / 4> + TAddGI (csd.hpp, fft.hpp:63-105): 160 COMPLEX16 samples of one chain from the transformed buffer, output sample i = time sample
// (i + 96 - csd) & 127.  Lane e stores samples 4e..4e+3 and, for e < 8, the same words once more as 128+4e..+3 (the index is the same modulo 128), as 16-byte
// words where the stream allows; word by word otherwise.
template <bool SWZ>
__device__ __forceinline__ void tx_emit160(const uint32_t* s, int e, uint32_t* o, int csd)
{
    if ((reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
        const uint32_t n0 = (uint32_t)(4 * e + 96 - csd);
        uint4 v;
        v.x = tx_tsample<SWZ>(s, n0); v.y = tx_tsample<SWZ>(s, n0 + 1); v.z = tx_tsample<SWZ>(s, n0 + 2); v.w = tx_tsample<SWZ>(s, n0 + 3);
        reinterpret_cast<uint4*>(o)[e] = v;
        if (e < 8) reinterpret_cast<uint4*>(o)[32 + e] = v;
    } else {                                                                     // (a frame placed at a sample offset that is not a multiple of four)
        for (int i = e; i < 160; i += 32) o[i] = tx_tsample<SWZ>(s, (uint32_t)(i + 96 - csd));
    }
}

// ---- the short guard interval of the 40 MHz HT pair (k_tx_ht40.hip): 144 COMPLEX16 samples of one chain from the transformed buffer, output
// sample i = time sample (i + 112) & 127 -- the last 16 of the 128, then the 128; no cyclic shift.  36 16-byte words where the stream allows: lane e stores word e and,
// for e < 4, the same word once more as word 32 + e (the index is the same modulo 128); word by word otherwise.  144 samples are 576 bytes: a frame that starts
// 16-byte aligned keeps every data symbol on the vector path.
template <bool SWZ>
__device__ __forceinline__ void tx_emit144(const uint32_t* s, int e, uint32_t* o)
{
    if ((reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
        const uint32_t n0 = (uint32_t)(4 * e + 112);
        uint4 v;
        v.x = tx_tsample<SWZ>(s, n0); v.y = tx_tsample<SWZ>(s, n0 + 1); v.z = tx_tsample<SWZ>(s, n0 + 2); v.w = tx_tsample<SWZ>(s, n0 + 3);
        reinterpret_cast<uint4*>(o)[e] = v;
        if (e < 4) reinterpret_cast<uint4*>(o)[32 + e] = v;
    } else {
        for (int i = e; i < 144; i += 32) o[i] = tx_tsample<SWZ>(s, (uint32_t)(i + 112));
    }
}

// ---- the fixed fields of an HT-mixed frame from the per-device table [2 chains][1120]: samples 0..639 (L-STF, L-LTF) and 1120..1599 (HT-STF, HT-LTF1,
// HT-LTF2) of both chains; the three SIG symbols go between them
static_assert(kTx11nPreamble == 1120 && kTxHt40Preamble == 1120, "one table shape for both HT transmitters");
__device__ __forceinline__ void tx_copy_fixed_fields(const uint32_t* table, uint32_t* out0, uint32_t* out1, int tid)
{
#pragma unroll
    for (int ch = 0; ch < 2; ch++) {
        const uint32_t* src = table + ch * 1120;
        uint32_t* o = ch ? out1 : out0;
        if ((reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
            for (int i = tid; i < 1120 / 4; i += 256)
                reinterpret_cast<uint4*>(o + (i < 160 ? 0 : 480))[i] = reinterpret_cast<const uint4*>(src)[i];
        } else {
            for (int i = tid; i < 1120; i += 256) o[i < 640 ? i : i + 480] = src[i];
        }
    }
}

}  // namespace sora
