// k_tx.hip -- 802.11a transmitter on the GPU: the modulation graph
//   TBB11aSrc -> T11aSc -> TBB11aMRSelect -> TConvEncode_{12,23,34} -> T11aInterleave* -> TMap11a* -> T11aAddPilot
//   -> TIFFTx -> TPackSample16to8 -> TModSink          (kernel/bb/demod11/fb11amod_config.hpp:74-110)
// plus the preamble source (kernel/bb/Brick11/src/preamble11a.hpp:19-140).  Output: COMPLEX8 at 40 MHz, what
// `demod11 -m` writes -- or, k_tx11a<true>, at 44 MHz: CreateModGraph11a_44M / CreatePreamble11a_44M, the same graphs with TUpsample40MTo44M
// (Brick11/src/sampling.hpp:8-32, 40MTo44M.hpp) in front of TPackSample16to8, what the reference's radio applications send.  Every stage is data-parallel once restated:
//   * scrambler (scramble.hpp:237-251): the register sequence is a phase of one period-127 cycle -> two table reads
//   * convolutional encoder (conv_enc.hpp:6-14): coded bit = xor of five of the last seven input bits; the puncturing
//     patterns map a coded-bit index to (input bit, generator) in closed form
//   * interleaver (interleave.hpp:43-58): coded bit k -> position j(k), the table the receiver's de-interleaver reads
//   * FCS: the parallel CRC-32 of k_finish
// The bricks' arithmetic is dev_tx.h's; here are the frame geometry, the LDS plan, the 16 -> 8 bit emission and the 44 MHz resampler.
// One 256-thread block per frame; eight OFDM symbols per pass, 32 lanes each (IFFT<128>: 4 points per lane).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_tx.h"

namespace sora {

constexpr int kTx11aMpdu = kCrcWaveBytes;                   // the MPDU bytes k_tx11a's one-wave FCS and its LDS plan hold
__device__ __constant__ uint8_t kLtsPos[64] = {              // LTS_Positive_table (ieee80211const.h:23-28)
    0,1,0,0,1,1,0,1,0,1,0,0,0,0,0,1, 1,0,0,1,0,1,0,1,1,1,1,0,0,0,0,0,
    0,0,0,0,0,0,1,1,0,0,1,1,0,1,0,1, 1,1,1,1,1,0,0,1,1,0,1,0,1,1,1,1 };
constexpr int kBpskMod = 10720;                              // mapper11a.hpp:8-11
__device__ __forceinline__ int kmod_of(int nb) { return nb == 1 ? kBpskMod : nb == 2 ? (int)(kBpskMod / 1.414) : nb == 4 ? (int)(kBpskMod / 3.162) : (int)(kBpskMod / 6.481); }
__device__ __forceinline__ int sat8(int v) { return min(max(v, -128), 127); }          // _mm_packs_epi16 (stdbrick.hpp:430)

// 160 time samples of one OFDM symbol from its 64 frequency bins (TIFFTx, fft.hpp:21-59): bins 0..31 -> 0..31, 32..63 ->
// 96..127 of a 128-point IFFT, >> 4, GI = last 32, first/last two samples halved, saturating 16 -> 8 bit pack.
// s_bins: 128 words (zero outside the 64 bins); 32 lanes, e = lane of the group.
// The samples leave straight from where the IFFT's last stage put them: output sample i of a symbol is time sample n = (i + 96) & 127, at word brev7(n)
// (FFT128LUTMap) -- four per lane as one 8-byte store, the shift, the clamp (_mm_packs_epi16, stdbrick.hpp:430) and the byte pick on packed halves.  A lane's four
// samples in a row, i = 4 e + k, sit at brev5((e + 24) & 31) + 32 brev2(k); its one sample of the last 32, i = 128 + e, at 4 brev5(e) + 3.
struct EmitPlan { uint32_t a4, a1; uint32_t sh01, shs; };
__device__ __forceinline__ EmitPlan emit_plan(int e)
{
    EmitPlan P;
    P.a4 = __brev((unsigned)((e + 24) & 31)) >> 27;
    P.a1 = 4u * (__brev((unsigned)e) >> 27) + 3u;
    P.sh01 = e == 0 ? 0x00050005u : 0x00040004u;                                 // samples 0, 1 ...
    P.shs = e >= 30 ? 0x00050005u : 0x00040004u;                                 // ... and 158, 159 are halved
    return P;
}
__device__ __forceinline__ uint32_t pk_sra_clamp8(uint32_t v, uint32_t sh)
{
    const s16x2_t lo = { (short)-128, (short)-128 }, hi = { (short)127, (short)127 };
    const s16x2_t x = __builtin_bit_cast(s16x2_t, v) >> __builtin_bit_cast(s16x2_t, sh);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_elementwise_max(x, lo), hi));
}
// TUpsample40MTo44M (40MTo44M.hpp:66-125) on one 160-sample block x -> 176 samples y, in 16 bits, no state between blocks.  In closed form, with
//   mh(a, c) = (a c + 16384) >> 15 (_mm_mulhrs_epi16, I and Q apart) and S(k) = floor(32767 k / 11) (S1(), 40MTo44M.hpp:12):  for j = 11 m + r, r = 0..10,
//   y[j] = int16(mh(x[j - m - 1], S(r)) + mh(x[j - m], S(11 - r)))          (S(0) = 0, S(11) = 32767: y[11 m] = mh(x[10 m], 32767))
// y[175] asks for x[160]: the reference loads it from behind its input (40MTo44M.hpp:112); here a block ends in x[160] = 0 unless the same
// pin-queue burst holds the next block (the preamble's blocks 0..2).
__device__ __forceinline__ int mulhrs(int a, int c) { return (a * c + 16384) >> 15; }
__device__ __forceinline__ uint32_t up44_mix(uint32_t lo, uint32_t hi, int r)    // -> COMPLEX8 in the low 16 bits (the clamp of TPackSample16to8 comes last)
{
    const int cl = r * 32767 / 11, ch = (11 - r) * 32767 / 11;
    const int re = (short)(mulhrs((short)lo, cl) + mulhrs((short)hi, ch)), im = (short)(mulhrs((int)lo >> 16, cl) + mulhrs((int)hi >> 16, ch));
    return (uint32_t)(sat8(re) & 255) | ((uint32_t)(sat8(im) & 255) << 8);
}
// sample i of the 40 MHz symbol as TIFFTx hands it on (16 bits, shifted), read where the IFFT's last stage left it; 0 behind the symbol
__device__ __forceinline__ uint32_t x40_at(const uint32_t* s_bins, int i)
{
    const uint32_t sh = (i < 2 || i >= 158) ? 0x00050005u : 0x00040004u;
    const s16x2_t v = __builtin_bit_cast(s16x2_t, s_bins[brev7((uint32_t)(i + 96) & 127u)]) >> __builtin_bit_cast(s16x2_t, sh);
    return i >= 160 ? 0u : __builtin_bit_cast(uint32_t, v);
}
// 44 MHz samples 4 w .. 4 w + 3 of the symbol (w = 0..43) as one 8-byte word: they lie between five 40 MHz samples in a row
__device__ __forceinline__ uint2 up44_word(const uint32_t* s_bins, int w)
{
    const int j0 = 4 * w, base = j0 - j0 / 11;
    uint32_t v[5], b[4];
#pragma unroll
    for (int t = 0; t < 5; t++) v[t] = x40_at(s_bins, base - 1 + t);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = j0 + k, m = j / 11, r = j - 11 * m;
        const bool step = j - m - base == k;                                     // (false once a multiple of 11 lies in j0 + 1 .. j: there the input index stands still)
        b[k] = up44_mix(step || k == 0 ? v[k] : v[k - 1], step || k == 0 ? v[k + 1] : v[k], r);
    }
    return make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
}
template <bool UP44>
__device__ __forceinline__ void ifft_emit(uint32_t* s_bins, int e, const Fft128Tw& tw, const EmitPlan& P, int8_t* out8)
{
    tx_ifft128<false>(s_bins, e, tw);
    if (out8 == nullptr) return;                                                 // (a group past the last symbol only keeps the barriers company)
    if constexpr (UP44) {                                                        // 176 samples = 44 words of 8 bytes: one per lane, then 12 more
        if ((reinterpret_cast<uintptr_t>(out8) & 7u) == 0) {
            reinterpret_cast<uint2*>(out8)[e] = up44_word(s_bins, e);
            if (e < 12) reinterpret_cast<uint2*>(out8)[32 + e] = up44_word(s_bins, 32 + e);
        } else {
            for (int j = e; j < 176; j += 32) {
                const int m = j / 11;
                reinterpret_cast<uint16_t*>(out8)[j] = (uint16_t)up44_mix(x40_at(s_bins, j - m - 1), x40_at(s_bins, j - m), j - 11 * m);
            }
        }
        return;
    }
    if ((reinterpret_cast<uintptr_t>(out8) & 7u) == 0) {
        const uint32_t w0 = pk_sra_clamp8(s_bins[P.a4], P.sh01), w1 = pk_sra_clamp8(s_bins[P.a4 + 64], P.sh01);
        const uint32_t w2 = pk_sra_clamp8(s_bins[P.a4 + 32], 0x00040004u), w3 = pk_sra_clamp8(s_bins[P.a4 + 96], 0x00040004u), w4 = pk_sra_clamp8(s_bins[P.a1], P.shs);
        uint2 o;                                                                 // low bytes of (re0, im0, re1, im1)
        o.x = __builtin_amdgcn_perm(w1, w0, 0x06040200u); o.y = __builtin_amdgcn_perm(w3, w2, 0x06040200u);
        reinterpret_cast<uint2*>(out8)[e] = o;
        reinterpret_cast<uint16_t*>(out8)[128 + e] = (uint16_t)__builtin_amdgcn_perm(0u, w4, 0x0c0c0200u);
    } else {                                                                     // (a frame the caller placed at a sample offset that is not a multiple of four)
        for (int i = e; i < 160; i += 32) {
            const uint32_t w = pk_sra_clamp8(s_bins[brev7((uint32_t)(i + 96) & 127u)], (i < 2 || i >= 158) ? 0x00050005u : 0x00040004u);
            reinterpret_cast<uint16_t*>(out8)[i] = (uint16_t)__builtin_amdgcn_perm(0u, w, 0x0c0c0200u);
        }
    }
}

// The 640-sample preamble (preamble11a.hpp:19-100), computed once per device into a table, and the 704 samples of its 44 MHz form.
__global__ void __launch_bounds__(64) k_tx_preamble(int8_t* out8, int8_t* out44, Tables T)
{
    __shared__ uint32_t s_f[2][128];
    __shared__ uint32_t s_t[2][128];
    __shared__ uint32_t s_lut[640];
    const int g = threadIdx.x >> 5, e = threadIdx.x & 31;
    auto sync = []() { __syncthreads(); };
    for (int i = e; i < 128; i += 32) s_f[g][i] = 0;
    sync();
    if (g == 0 && e == 0) {                                                      // short training symbol: 12 carriers
        const int m = (int)(uint16_t)(1.0 * kBpskMod * 1.472);
        const int idx[12] = { 4, 8, 12, 16, 20, 24, 104, 108, 112, 116, 120, 124 };
        const int sg[12]  = { -1, -1, 1, 1, 1, 1, 1, -1, 1, -1, -1, 1 };
        for (int k = 0; k < 12; k++) { const int v = w16(sg[k] * m); s_f[0][idx[k]] = pack(mk(v, v)); }
    }
    if (g == 1) {                                                                // long training symbol
        for (int i = 1 + e; i <= 26; i += 32) s_f[1][i] = pack(mk(kLtsPos[i] ? kBpskMod : -kBpskMod, 0));
        for (int i = 64 - 26 + e; i < 64; i += 32) s_f[1][i + 64] = pack(mk(kLtsPos[i] ? kBpskMod : -kBpskMod, 0));
    }
    sync();
    cpx x[4], y[4];
#pragma unroll
    for (int m = 0; m < 4; m++) x[m] = unpack(s_f[g][e + 32 * m]);
    fft128_group<true>(x, y, s_f[g], e, T, sync);
#pragma unroll
    for (int q = 0; q < 4; q++) s_t[g][e + 32 * q] = pack(sra(y[q], 4));
    sync();
    // STS: 128 samples repeated periodically over 320; LTS: GI2 (last 64 of the symbol) + two copies of 128
    for (int i = threadIdx.x; i < 320; i += 64) s_lut[i] = s_t[0][i & 127];
    for (int i = threadIdx.x; i < 256; i += 64) s_lut[320 + 64 + i] = s_t[1][i & 127];
    for (int i = threadIdx.x; i < 64; i += 64) s_lut[320 + i] = s_t[1][64 + i];
    sync();
    for (int i = threadIdx.x; i < 640; i += 64) {
        cpx v = unpack(s_lut[i]);
        if (i == 0 || i == 1 || i == 318 || i == 319 || i == 320 || i == 321 || i == 638 || i == 639) v = sra(v, 1);
        out8[2 * i] = (int8_t)sat8(v.re); out8[2 * i + 1] = (int8_t)sat8(v.im);
        s_lut[i] = pack(v);
    }
    sync();
    // CreatePreamble11a_44M: TUpsample40MTo44M over the four 160-sample blocks of the 16-bit preamble, before the clamp.  The source hands all 640 samples on as one
    // burst, so blocks 0..2 find the next block's first sample behind their last one; block 3 ends in x[160] = 0.
    for (int j = threadIdx.x; j < 704; j += 64) {
        const int blk = j / 176, jj = j - 176 * blk, m = jj / 11, hi = 160 * blk + jj - m;
        reinterpret_cast<uint16_t*>(out44)[j] = (uint16_t)up44_mix(s_lut[max(hi - 1, 0)], hi < 640 ? s_lut[hi] : 0u, jj - 11 * m);
    }
}

// UP44: COMPLEX8 at 44 MHz -- A.preamble is the 704-sample table, A.out_off counts 44 MHz samples, a symbol is 176 samples.  Everything up to the IFFT is one code.
// The 44 MHz form keeps its two words' addresses, weights and selects in registers across the symbol loop (98 of them): four workgroups per CU without scratch,
// where eight would spill 50 dwords; the 40 MHz form stays at eight.
template <bool UP44>
__global__ void __launch_bounds__(256, UP44 ? 4 : 8) k_tx11a(TxArgs A)
{
    constexpr int kPre = UP44 ? 704 : 640, kSym = UP44 ? 176 : 160;
    // The LDS plan holds the MPDU one wave's FCS covers (kTx11aMpdu): SERVICE(2) + MPDU + FCS(4) + tail(1), at most 27 pad bytes (one symbol at
    // 54 Mbps), the 8 bytes the loader clears behind them; a generator word per four field bytes.
    static_assert(2 + kTx11aMpdu + 4 + 1 + 27 + 8 <= 2608 && (2 + kTx11aMpdu + 4 + 1 + 27 + 3) / 4 <= 656, "LDS plan");
    __shared__ alignas(4) uint8_t s_data[2608];
    // generator outputs A (133) / B (171) of the whole data field, bit i of the stream = bit i & 31 of word i >> 5
    __shared__ uint32_t s_gab[2][656];
    uint32_t* const s_ga = s_gab[0]; uint32_t* const s_gb = s_gab[1];
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_z[6 * 8 * 16];
    __shared__ uint32_t s_bins[8][128];
    // the interleaver inverted: position -> coded bit of the symbol, for the frame's modulation and for the SIGNAL symbol (BPSK)
    __shared__ uint16_t s_inv[288 + 48];
    __shared__ uint32_t s_fcs;
    // interleaver positions of the frame's modulation, then of the SIGNAL symbol (BPSK)
    __shared__ uint16_t s_map[288 + 48];
    const uint32_t f = blockIdx.x;
    const int tid = threadIdx.x, g = tid >> 5, e = tid & 31;
    const Tables& T = A.T;
    const uint32_t L = A.len[f], kbps = A.rate[f];
    const uint8_t* mp = A.mpdu + A.off[f];
    int8_t* out = A.out8 + A.out_off[f] * 2;
    int nb, cr, nd, rc;
    switch (kbps) {                                                              // ieee80211a_cmn.h:65-149, ieee80211const.h:3-10
    case 6000:  nb = 1; cr = 0; nd = 24;  rc = 0xB; break;  case 9000:  nb = 1; cr = 2; nd = 36;  rc = 0xF; break;
    case 12000: nb = 2; cr = 0; nd = 48;  rc = 0xA; break;  case 18000: nb = 2; cr = 2; nd = 72;  rc = 0xE; break;
    case 24000: nb = 4; cr = 0; nd = 96;  rc = 0x9; break;  case 36000: nb = 4; cr = 2; nd = 144; rc = 0xD; break;
    case 48000: nb = 6; cr = 1; nd = 192; rc = 0x8; break;  default:    nb = 6; cr = 2; nd = 216; rc = 0xC; break;
    }
    // TBB11aSrc::Process (PHY_11a.hpp:132-202): SERVICE(2) + MPDU + FCS(4) + tail(1) + pad; rate 9 pads to two symbols
    const uint32_t ndp = kbps == 9000 ? (uint32_t)nd * 2 : (uint32_t)nd;
    const uint32_t dbytes = 2 + (L + 4) + 1;
    const uint32_t rem = (dbytes * 8) % ndp, pad_bits = rem ? ndp - rem : 0;
    const uint32_t nbytes = dbytes + (pad_bits + 7) / 8;
    const uint32_t nsym = nbytes * 8 / (uint32_t)nd;

    s_crc[tid] = T.crc[tid];
    for (int i = tid; i < 6 * 8 * 16; i += 256) s_z[i] = T.crcz[i];
    // (+ 8: the word-wise encoder reads up to 3 bytes past nbytes)
    for (uint32_t i = tid; i < nbytes + 8; i += 256) s_data[i] = (i >= 2 && i < 2 + L) ? mp[i - 2] : (uint8_t)0;
    __syncthreads();
    if (tid < 64) tx_fcs_waves<1>(s_data + 2, L, s_crc, s_z, tid, &s_fcs);      // FCS of the MPDU: one wave
    __syncthreads();
    if (tid < 4) s_data[2 + L + tid] = (uint8_t)(tx_fcs_join<1>(s_z, &s_fcs) >> (8 * tid));
    __syncthreads();
    tx_scramble(s_data, nbytes, dbytes - 1, T.scr_phase[A.seed[f] >> 1], T, tid);   // T11aSc: the register holds the previous 8 output bits
    for (int i = tid; i < kPre; i += 256) reinterpret_cast<uint16_t*>(out)[i] = reinterpret_cast<const uint16_t*>(A.preamble)[i];
    __syncthreads();
    // TConvEncode_* over the whole field
    for (uint32_t w = tid; w < (nbytes + 3) / 4; w += 256) tx_encode_word(reinterpret_cast<const uint32_t*>(s_data), w, 0xFFFFFFFFu, s_ga[w], s_gb[w]);
    __syncthreads();

    const uint32_t sig = tx_lsig((uint32_t)rc, L + 4);                           // PLCP SIGNAL
    // From here on every LDS slice is private to a 32-lane group (half a wave): a wave-level barrier orders what the groups of a wave
    // write and read, the waves of the block run free of each other.
    for (int i = tid; i < 48 * nb; i += 256) s_map[i] = T.deint[(nb == 1 ? 0 : nb == 2 ? 1 : nb == 4 ? 2 : 3) * 288 + i];
    if (tid < 48) s_map[288 + tid] = T.deint[tid];
    const Fft128Tw tw = fft128_twiddles(T, e);
    __syncthreads();
    for (int k = tid; k < 48 * nb; k += 256) s_inv[s_map[k]] = (uint16_t)k;
    if (tid < 48) s_inv[288 + s_map[288 + tid]] = (uint16_t)tid;
    __syncthreads();
    // The mapper reads its bits where the encoder left them.  A symbol is 96 components (carrier c, I or Q; 48 for BPSK), three per lane of the symbol's 32:
    // component q = e + 32 t.  Its M bits sit at interleaved positions c N_BPSC + h M + m, i.e. are coded bits k = inverse(position) of the symbol, and coded bit k of
    // a symbol is generator `which` at input bit (s - 1) N_DBPS + il -- (il, which) follow from k and the puncturing pattern and do NOT depend on the symbol (N_CBPS is a
    // whole number of puncture periods, tx_punct_offset).
    const int M = nb == 1 ? 1 : nb / 2;
    // (registers, not a packed word: the loop below neither unpacks nor recomputes anything that depends on the lane alone)
    // bit offset within s_gab of each of the component's bits at symbol 0: input bit within the symbol + 656 * 32 for generator B (a whole number of words)
    uint32_t il[3][3], ES[2] = { 0, 0 };
    uint32_t cw[3];                                                              // byte address of the component's 16-bit half in the symbol's bins
    // TMap11a* + T11aAddPilot (mapper11a.hpp, pilot.hpp:76-118): carriers in the order -26..-1, +1..+26 without pilots (carrier_bin48)
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const int q = e + 32 * t;
#pragma unroll
        for (int m = 0; m < 3; m++) il[t][m] = 0;
        if (nb == 1) {
            if (t < 2 && q < 48) il[t][0] = tx_punct_offset(cr, s_inv[q], 656u * 32u);
            cw[t] = (uint32_t)bin128(carrier_bin48(t < 2 && q < 48 ? q : 0)) * 4u;
        } else {
            const int c = q >> 1, h = q & 1;
#pragma unroll
            for (int m = 0; m < 3; m++) if (m < M) il[t][m] = tx_punct_offset(cr, s_inv[c * nb + h * M + m], 656u * 32u);
            cw[t] = (uint32_t)bin128(carrier_bin48(c)) * 4u + 2u * (uint32_t)h;
        }
        if (t < 2 && q < 48) { const int k = s_inv[288 + q]; ES[t] = (uint32_t)(k >> 1) | ((uint32_t)(k & 1) << 8); }
    }
    const EmitPlan plan = emit_plan(e);
    const int kmod = kmod_of(nb), lvl0 = -((1 << M) - 1) * kmod, kmod2 = 2 * kmod;
    const uint32_t total = 1 + nsym;                                             // SIGNAL + data symbols
    const uint32_t* const gab = &s_gab[0][0];
    char* const bins = reinterpret_cast<char*>(s_bins[g]);
    for (uint32_t s0 = 0; s0 < total; s0 += 8) {
        const uint32_t s = s0 + (uint32_t)g;
        const bool active = s < total;
        const bool is_sig = s == 0;
        for (int i = e; i < 128; i += 32) s_bins[g][i] = 0;
        if (active) {
            if (is_sig) {
                // the SIGNAL symbol: rate 1/2 over the 24 header bits (encoder state 0), BPSK
                const uint32_t A_ = sig ^ (sig << 2) ^ (sig << 3) ^ (sig << 5) ^ (sig << 6), B_ = sig ^ (sig << 1) ^ (sig << 2) ^ (sig << 3) ^ (sig << 6);
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const int c = e + 32 * t;
                    if (c < 48) { const unsigned bit = (((ES[t] >> 8) ? B_ : A_) >> (ES[t] & 255u)) & 1u; s_bins[g][bin128(carrier_bin48(c))] = pack(mk(bit ? kBpskMod : -kBpskMod, 0)); }
                }
            } else {
                const uint32_t ibase = (s - 1u) * (uint32_t)nd;
                if (nb == 1) {
#pragma unroll
                    for (int t = 0; t < 2; t++)
                        if (e + 32 * t < 48) *reinterpret_cast<uint32_t*>(bins + cw[t]) = pack(mk(tx_gen_bit(gab, ibase + il[t][0]) ? kBpskMod : -kBpskMod, 0));
                } else {
#pragma unroll
                    for (int t = 0; t < 3; t++) *reinterpret_cast<uint16_t*>(bins + cw[t]) = (uint16_t)tx_axis_level(gab, ibase, il[t], M, kmod2, lvl0);
                }
            }
            if (e < 4) {
                const unsigned pidx = is_sig ? 127u : (unsigned)((s - 1) % 127u);   // m_PilotIndex 127 -> 0 after SIGNAL (pilot.hpp:66-69)
                tx_put_pilots11a(s_bins[g], e, pilot_sgn(pidx) ? -kBpskMod : kBpskMod);
            }
        }
        ifft_emit<UP44>(s_bins[g], e, tw, plan, active ? out + 2 * (kPre + kSym * (size_t)s) : (int8_t*)nullptr);
        wave_lds_sync();
    }
}
template __global__ void k_tx11a<false>(TxArgs A);
template __global__ void k_tx11a<true>(TxArgs A);

}  // namespace sora
