// k_tx11n.hip -- 802.11n 2x2 transmitter on the GPU (MCS 8..14, 20 MHz, long GI): the reference's three modulation graphs as
// Test11N_FB_Mod drives them (kernel/bb/demod11/fb11nmod_config.hpp, fb11n_mod.cpp:28-70), one frame after the other:
//   preamble  LSrc / HTSrc (preamble11n.hpp): L-STF, L-LTF | HT-STF, HT-LTF1, HT-LTF2 -- a table built once per device on the host
//   SIG       TBB11nSigSrc -> TConvEncode_12 -> T11aInterleaveBPSK -> TSigMap11n (L-SIG on I, HT-SIG on Q) -> T11aAddPilot<30339>
//             -> TIFFTxOnly -> chain 0 TAddGI, chain 1 TCSD<2> + TAddGI
//   data      TBB11nSrc -> T11aSc -> TBB11nMRSelect -> TConvEncode_{12,23,34} -> TStreamParser*_12 -> T11nInterleave*_S1/_S2
//             -> TMap11a* (30339 / 21453 / 9594 / 4681) -> T11nAddPilot<0/1> -> TIFFTxOnly -> chain 1 TCSD<4> -> TAddGI
// Output: two COMPLEX16 streams at 40 MHz, GetSinkSampleCount() samples each.  Every stage restated as an index map:
//   * scrambler, encoder and puncturing: as k_tx.hip (the same bricks), over nvalid input bits; coded bits past the encoder's
//     last group are the stream parser's zero padding (tx11n_plan in kernels.h)
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
#include "dev_pilot11a.h"
#include "dev_11n.h"

namespace sora {

namespace {
constexpr int kWords = 1056;                // generator words per stream: nsym * NDBPS input bits of a 4092-byte MPDU is at most 33696 (MCS 14)
constexpr int kBpsk11n = 30339;             // fb11nmod_config.hpp: TMap11aBPSK<30339>, T11nAddPilot, T11aAddPilot<30339>, TSigMap11n
__device__ __forceinline__ int kmod11n(int nb) { return nb == 1 ? kBpsk11n : nb == 2 ? 21453 : nb == 4 ? 9594 : 4681; }
__device__ __forceinline__ uint32_t brev7(uint32_t n) { return __brev(n) >> 25; }
// 48 carriers of the legacy SIG symbols (T11aAddPilot::add_pilot, pilot.hpp:76-96): -26..-1 then 1..26 without pilots, 128-point grid
__device__ __forceinline__ int sig_bin128(int c)
{
    int bin;
    if (c < 24) { bin = 38 + c; if (bin >= 43) bin++; if (bin >= 57) bin++; } else { bin = 1 + (c - 24); if (bin >= 7) bin++; if (bin >= 21) bin++; }
    return bin < 32 ? bin : bin + 64;
}

// 160 samples of one chain from the IFFT's output (time sample n at word brev7(n)): output sample i is time sample (i + 96 - csd) & 127.
// Lane e stores samples 4e..4e+3 and, for e < 8, 128+4e..+3 as 16-byte words where the stream allows; word by word otherwise.
__device__ __forceinline__ void emit_chain(const uint32_t* s, int e, uint32_t* o, int csd)
{
    if ((reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
        const uint32_t n0 = (uint32_t)(4 * e + 96 - csd);
        uint4 v;
        v.x = s[brev7(n0 & 127u)]; v.y = s[brev7((n0 + 1) & 127u)]; v.z = s[brev7((n0 + 2) & 127u)]; v.w = s[brev7((n0 + 3) & 127u)];
        reinterpret_cast<uint4*>(o)[e] = v;
        if (e < 8) {
            const uint32_t n1 = n0 + 128;
            v.x = s[brev7(n1 & 127u)]; v.y = s[brev7((n1 + 1) & 127u)]; v.z = s[brev7((n1 + 2) & 127u)]; v.w = s[brev7((n1 + 3) & 127u)];
            reinterpret_cast<uint4*>(o)[32 + e] = v;
        }
    } else {                                                                     // (a frame placed at a sample offset that is not a multiple of four)
        for (int i = e; i < 160; i += 32) o[i] = s[brev7((uint32_t)(i + 96 - csd) & 127u)];
    }
}
template <typename SYNC>
__device__ __forceinline__ void ifft_emit2(uint32_t* s, int e, const Fft128Tw& tw, uint32_t* o0, int csd0, uint32_t* o1, int csd1, SYNC sync)
{
    pcx x[4];
    sync();
#pragma unroll
    for (int m = 0; m < 4; m++) x[m] = s[e + 32 * m];
    ifft128_core_pk(x, s, e, tw, sync);                                          // IFFT<128> on packed COMPLEX16 (bit-exact with fft128_core<true>)
    if (o0) emit_chain(s, e, o0, csd0);                                          // (a group past the last symbol only keeps the barriers company)
    if (o1) emit_chain(s, e, o1, csd1);
}
// the register after m = 40 * 2^k zero bytes (crc32_wave's tree tables)
__device__ __forceinline__ uint32_t crc_zeros(const uint32_t* s_z, int k, uint32_t c)
{
    uint32_t z = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) z ^= s_z[(k * 8 + q) * 16 + ((c >> (4 * q)) & 15u)];
    return z;
}
}  // namespace

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
    if (tid < 128) {                                                             // FCS (CF_11nTxVector::crc32 = CalcCRC32 of the MPDU)
        if (L >= 4) {
            // two waves of crc32_wave: lanes 64..127 take the 2560 bytes before the last 2560; CRC(0, M1 | M2) = Z_2560(CRC(0, M1)) ^ CRC(0, M2)
            const uint32_t c = crc32_wave(s_data + 2, (int)L, s_crc, s_z, tid);
            if ((tid & 63) == 0) s_crcw[tid >> 6] = c;
        } else if (tid == 0) {
            uint32_t c = 0xFFFFFFFFu;
            for (uint32_t i = 0; i < L; i++) c = (c >> 8) ^ s_crc[(s_data[2 + i] ^ c) & 0xFF];
            s_crcw[0] = c; s_crcw[1] = 0;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const uint32_t fcs = ~(crc_zeros(s_z, 5, crc_zeros(s_z, 5, s_crcw[1])) ^ s_crcw[0]);
        for (int k = 0; k < 4; k++) s_data[2 + L + k] = (uint8_t)(fcs >> (8 * k));
    }
    __syncthreads();
    {   // T11aSc (scramble.hpp:233-258) with DO_SCRAMBLE, TAIL_SCRAMBLE on the tail byte: it keeps only its two pad bits
        const unsigned s7 = (A.seed ? A.seed[f] : 0xABu) >> 1;
        const unsigned phase = T.scr_phase[s7];                                  // 255: the all-zero state stays zero
        const uint32_t tail = 2 + L + 4;
        for (uint32_t i = tid; i < P.nbytes; i += 256) {
            unsigned c = s_data[i] ^ (phase == 255 ? 0u : T.scr_seq[(phase + 8u * i) % 127u]);
            if (i == tail) c &= 0xC0u;
            s_data[i] = (uint8_t)c;
        }
    }
    // the fixed fields (LSrc, HTSrc) from the per-device table: samples 0..639 and 1120..1599 of both chains
#pragma unroll
    for (int ch = 0; ch < 2; ch++) {
        const uint32_t* src = A.preamble + ch * kTx11nPreamble;
        uint32_t* o = ch ? out1 : out0;
        if ((reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
            for (int i = tid; i < (int)kTx11nPreamble / 4; i += 256)
                reinterpret_cast<uint4*>(o + (i < 160 ? 0 : 480))[i] = reinterpret_cast<const uint4*>(src)[i];
        } else {
            for (int i = tid; i < (int)kTx11nPreamble; i += 256) o[i < 640 ? i : i + 480] = src[i];
        }
    }
    __syncthreads();
    // TConvEncode_* 32 input bits at a time (k_tx.hip): A = x ^ x>>2 ^ x>>3 ^ x>>5 ^ x>>6, B = x ^ x>>1 ^ x>>2 ^ x>>3 ^ x>>6 (x>>k: k bits earlier)
    {
        const uint32_t* dw = reinterpret_cast<const uint32_t*>(s_data);
        for (uint32_t w = tid; w < nw; w += 256) {
            const uint32_t X = dw[w], Pw = w ? dw[w - 1] : 0u;
            auto sh = [&](int k) { return (X << k) | (Pw >> (32 - k)); };
            const uint32_t x2 = sh(2), x3 = sh(3), x6 = sh(6);
            const uint32_t keep = 32 * w + 32 <= P.nvalid ? 0xFFFFFFFFu : (32 * w >= P.nvalid ? 0u : (1u << (P.nvalid - 32 * w)) - 1u);
            s_gab[0][w] = (X ^ x2 ^ x3 ^ sh(5) ^ x6) & keep;
            s_gab[1][w] = (X ^ sh(1) ^ x2 ^ x3 ^ x6) & keep;
        }
    }
    for (int k = tid; k < 52 * nb; k += 256) {
        s_inv[0][deint11n_index(nb, 0, k)] = (uint16_t)k;
        s_inv[1][deint11n_index(nb, 1, k)] = (uint16_t)k;
    }
    if (tid < 48) s_sinv[T.deint[tid]] = (uint8_t)tid;                           // T.deint[0..47]: the 11a BPSK interleaver, coded bit -> position
    const Fft128Tw tw = fft128_twiddles(T, e);
    __syncthreads();

    auto sync = []() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); };
    // L-SIG + HT-SIG (TBB11nSigSrc, _b_lsig.h, _b_htsig.h): 72 bits, rate 1/2 from state 0, three BPSK symbols of 48 coded bits
    if (g < 2 * 2) {                                                             // waves 0 and 1: groups 0..2 carry the three symbols
        uint32_t lsig = 0xBu | ((((P.nstd + 5) * 24 - 16 - 6) / 8) << 5);       // 6 Mbps, the length that spans the HT frame's symbols
        lsig |= (uint32_t)(__popc(lsig) & 1) << 17;
        const uint32_t ht_len = L + 4;
        const uint32_t h4 = (A.mcs[f] & 0x7Fu) | ((ht_len & 0xFFFFu) << 8) | (3u << 24);   // MCS, CBW 20, LENGTH, smoothing, not sounding
        uint32_t crc = 0xFF;                                                     // CalcCRC8(cdata, 4, 2): reflected, poly 0xE0, over 34 bits
        for (int b = 0; b < 34; b++) { crc ^= b < 32 ? (h4 >> b) & 1u : 0u; crc = (crc & 1u) ? (crc >> 1) ^ 0xE0u : crc >> 1; }
        crc = ~crc & 0xFFu;
        const uint64_t ht = (uint64_t)h4 | ((uint64_t)crc << 34);                   // NES 0, CRC bits 34..41, tail 0
        const uint64_t lo = (uint64_t)lsig | (ht << 24);                         // bits 0..63 of the 72-bit stream
        const uint32_t hi = (uint32_t)(ht >> 40);                                // bits 64..71
        auto bit = [&](int i) -> uint32_t { return i < 0 ? 0u : i < 64 ? (uint32_t)(lo >> i) & 1u : (hi >> (i - 64)) & 1u; };
        const int s = g;
        uint32_t* const bins = s_bins[g];
        for (int i = e; i < 128; i += 32) bins[i] = 0;
        if (s < 3) {
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int c = e + 32 * t;
                if (c < 48) {
                    const int kg = 48 * s + s_sinv[c], i = kg >> 1;
                    const uint32_t v = (kg & 1) ? bit(i) ^ bit(i - 1) ^ bit(i - 2) ^ bit(i - 3) ^ bit(i - 6) : bit(i) ^ bit(i - 2) ^ bit(i - 3) ^ bit(i - 5) ^ bit(i - 6);
                    const int a = v ? kBpsk11n : -kBpsk11n;
                    bins[sig_bin128(c)] = s == 0 ? pack(mk(a, 0)) : pack(mk(0, a));
                }
            }
            if (e < 4) {                                                         // T11aAddPilot: m_PilotIndex 127, 0, 1
                const unsigned pidx = s == 0 ? 127u : (unsigned)(s - 1);
                const uint32_t pw = pidx < 64 ? (pidx < 32 ? kPilotW0 : kPilotW1) : (pidx < 96 ? kPilotW2 : kPilotW3);
                const int p = (pw >> (pidx & 31u)) & 1u ? -kBpsk11n : kBpsk11n;
                const int bin = e == 0 ? 7 : e == 1 ? 21 : e == 2 ? 64 - 7 : 64 - 21;
                bins[bin < 32 ? bin : bin + 64] = pack(mk(e == 1 ? -p : p, 0));
            }
        }
        const bool on = s < 3;
        ifft_emit2(bins, e, tw, on ? out0 + 640 + 160 * s : nullptr, 0, on ? out1 + 640 + 160 * s : nullptr, 8, sync);
        sync();
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
        cw[t] = (uint32_t)(q < ncomp ? (nb == 1 ? 4 * data_bin(c) : 4 * data_bin(c) + 2 * h) : 0);
        cw[t] = (cw[t] >> 2) < 32 ? cw[t] : cw[t] + 4 * 64;                      // 64-bin grid -> 128 (TIFFTxOnly)
#pragma unroll
        for (int m = 0; m < 3; m++) {
            boff[t][m] = 0;
            if (q < ncomp && m < M) {
                const int k = s_inv[iss][c * nb + h * M + m];
                const int kc = ((k / S) * 2 + iss) * S + k % S;
                int il, which;
                if (P.cr == 0) { il = kc >> 1; which = kc & 1; }
                else if (P.cr == 1) { const int q3 = kc / 3, r = kc - 3 * q3; il = 2 * q3 + (r == 2); which = r == 1; }
                else { const int q4 = kc >> 2, r = kc & 3; il = 3 * q4 + (r == 2 ? 1 : r == 3 ? 2 : 0); which = r & 1; }
                boff[t][m] = (uint32_t)il + (uint32_t)which * (kWords * 32u);
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
            auto gen_bit = [&](uint32_t idx) -> uint32_t { return (gab[idx >> 5] >> (idx & 31u)) & 1u; };
            if (nb == 1) {
#pragma unroll
                for (int t = 0; t < 2; t++)
                    if (e + 32 * t < 52) *reinterpret_cast<uint32_t*>(binb + cw[t]) = pack(mk(gen_bit(ibase + boff[t][0]) ? kBpsk11n : -kBpsk11n, 0));
            } else {
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (e + 32 * t < 104) {
                        unsigned v = 0;                                         // first-transmitted bit = MSB (InitQamMapLut's reversal)
#pragma unroll
                        for (int m = 0; m < 3; m++) if (m < M) v |= gen_bit(ibase + boff[t][m]) << (M - 1 - m);
                        unsigned bb = v ^ (v >> 1); bb ^= bb >> 2;                // Gray -> binary (M <= 3)
                        *reinterpret_cast<uint16_t*>(binb + cw[t]) = (uint16_t)((int)bb * kmod2 + lvl0);
                    }
                }
            }
            if (e < 4) {
                // T11nAddPilot<iss> (pilot_11n.hpp:44-73, _b_dot11_pilot.h): pilot k of symbol n = polarity[(n + 3) % 127] x Psi_iss[(n + k) & 3],
                // Psi_0 = {1, 1, -1, -1}, Psi_1 = {1, -1, -1, 1}; k = 0..3 at carriers -21, -7, 7, 21
                const unsigned pidx = (s + 3u) % 127u;
                const uint32_t pw = pidx < 64 ? (pidx < 32 ? kPilotW0 : kPilotW1) : (pidx < 96 ? kPilotW2 : kPilotW3);
                const int j = (int)((s + (uint32_t)e) & 3u);
                const int psi = iss == 0 ? (j < 2 ? 1 : -1) : ((j == 0 || j == 3) ? 1 : -1);
                const int p = ((pw >> (pidx & 31u)) & 1u ? -psi : psi) * kBpsk11n;
                const int bin = e == 0 ? 64 - 21 : e == 1 ? 64 - 7 : e == 2 ? 7 : 21;
                bins[bin < 32 ? bin : bin + 64] = pack(mk(p, 0));
            }
        }
        ifft_emit2(bins, e, tw, active ? (iss ? out1 : out0) + 1600 + 160 * (size_t)s : nullptr, iss ? 16 : 0, nullptr, 0, sync);
        sync();
    }
}

}  // namespace sora
