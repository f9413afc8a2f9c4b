// k_11n.hip -- 802.11n 2x2, stage level: the bricks of the reference's 11n receive graph as batched per-stage entry points with
// the brick port shapes (sora_hip_*11n).  The whole-path graph is k_rx11n.hip, the 40 MHz data field k_ht40.hip; the bricks' arithmetic is stated once, in
// dev_11n.h, and a kernel here is a brick's piece behind its loads and in front of its stores.
//   sora_hip_demap11n         T11nDemap{BPSK,QPSK,QAM16,QAM64}        kernel/bb/Brick11/src/demapper11n.hpp:89-309 (dsp_demap.h)
//   sora_hip_deinterleave11n  T11nDeinterleave{...}_S0 / _S1           kernel/bb/Brick11/src/deinterleaver_11n.hpp:4-1618
//   sora_hip_mimo_est11n / _mimo_comp11n, _siso_est11n / _siso_comp11n, _sig_demap11n / _sig_decode11n, _cfo_est11n / _freq_comp11n, _pilot_track11n
//   sora_hip_cca11n (TCCA11n), _data_symbol11n, _stream_join11n, and the tail shared with the 802.11a graph, sora_hip_desc11a / _frame_sink11a
// Demap and de-interleave are pure gathers: one coalesced read of a symbol, table look-ups out of LDS, one coalesced write -- HBM-bound.
// The soft-value tables of dsp_demap.h are step functions of the limited coordinate v in [-128,127]; they are regenerated
// from their run lengths (value, count from v = -128 upward).  The de-interleavers are the standard HT interleaver
// (N_COL 13, N_ROW 4 N_BPSC, N_ROT 11) inverted, computed per element instead of the reference's unrolled tables.
#include "kernels.h"
#include "dev_11n.h"
#include "host_stage.h"

namespace sora {


// one wave per symbol, four symbols per block; lane l < 52 = data carrier l
__global__ void __launch_bounds__(256) k_demap11n_batch(const uint32_t* in, uint8_t* soft, int nb, uint32_t n)
{
    __shared__ uint8_t s_lut[6][256];
    fill_demap_luts(s_lut);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t sym = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sym >= n || lane >= 52) return;
    demap11n_store(soft + ((size_t)sym * 52 + lane) * nb, s_lut, unpack(in[(size_t)sym * 64 + data_bin(lane)]), nb);
}

// one thread per output soft value
__global__ void __launch_bounds__(256) k_deint11n_batch(const uint8_t* in, uint8_t* out, int nb, int iss, uint32_t n)
{
    const uint32_t per = 52u * nb;
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (uint64_t)n * per) return;
    const uint32_t sym = (uint32_t)(g / per); const int k = (int)(g - (uint64_t)sym * per);
    const int j = deint11n_index(nb, iss, k);
    out[g] = in[(uint64_t)sym * per + j];
}

// ---- TMimoChannelEst (channel_11n.hpp:329-443): one thread per carrier, 64 per frame

__global__ void __launch_bounds__(256) k_mimo_est11n_batch(const uint32_t* ltf0, const uint32_t* ltf1, uint32_t* h, uint32_t* hinv, uint32_t nframes)
{
    const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6); const int i = threadIdx.x & 63;
    if (f >= nframes) return;
    const int k = i < 32 ? i : i - 64;
    const bool negate = !(k >= -28 && k <= 28 && kHtLtf[k + 28] == 1);             // _80211n_HTLTFMask: every bin whose HT-LTF value is not +1
    const uint32_t* l0 = ltf0 + (size_t)f * 128; const uint32_t* l1 = ltf1 + (size_t)f * 128;
    cpx hh[2][2]; cf w[4];
    mimo_h_carrier(unpack(l0[i]), unpack(l0[i + 64]), unpack(l1[i]), unpack(l1[i + 64]), negate, hh);
#pragma unroll
    for (int r = 0; r < 2; r++) { h[((size_t)f * 2 + r) * 128 + i] = pack(hh[r][0]); h[((size_t)f * 2 + r) * 128 + 64 + i] = pack(hh[r][1]); }
    mimo_inverse(hh, w);
#pragma unroll
    for (int m = 0; m < 4; m++) hinv[(size_t)f * 256 + 64 * m + i] = mimo_weight_pack(w[m]);
}

// ---- TMimoChannelComp (channel_11n.hpp:445-521): x = (Hinv y) >> 9, saturating pack; one thread per carrier
__global__ void __launch_bounds__(256) k_mimo_comp11n_batch(const uint32_t* hinv, const uint32_t* frame_index, const uint32_t* y0, const uint32_t* y1,
                                                            uint32_t* x0, uint32_t* x1, uint32_t nsym)
{
    const uint32_t sidx = blockIdx.x * 4 + (threadIdx.x >> 6); const int i = threadIdx.x & 63;
    if (sidx >= nsym) return;
    const uint32_t* hi = hinv + (size_t)(frame_index ? frame_index[sidx] : 0u) * 256;
    const cpx a = unpack(y0[(size_t)sidx * 64 + i]), b = unpack(y1[(size_t)sidx * 64 + i]);
    x0[(size_t)sidx * 64 + i] = pack(mimo_comp_row(unpack(hi[i]), unpack(hi[64 + i]), a, b));
    x1[(size_t)sidx * 64 + i] = pack(mimo_comp_row(unpack(hi[128 + i]), unpack(hi[192 + i]), a, b));
}

// ---- TSisoChannelEst (channel_11n.hpp:33-231): one thread per (frame, RX chain, carrier)
__global__ void __launch_bounds__(256) k_siso_est11n_batch(const uint32_t* l0, const uint32_t* l1, uint32_t* ch, uint32_t nframes)
{
    const uint32_t f = blockIdx.x * 2 + (threadIdx.x >> 7); const int r = (threadIdx.x >> 6) & 1, i = threadIdx.x & 63;
    if (f >= nframes) return;
    ch[(size_t)f * 128 + r * 64 + i] = siso_est_carrier((r ? l1 : l0) + (size_t)f * 128, i);
}

// ---- TSisoChannelComp (channel_11n.hpp:233-297) + TMrcCombine (PHY_11n.hpp:362-398): x_r = sat((y_r * c_r) >> 9), mrc = (x_0 + x_1) >> 1
__global__ void __launch_bounds__(256) k_siso_comp11n_batch(const uint32_t* ch, const uint32_t* frame_index, const uint32_t* y0, const uint32_t* y1,
                                                            uint32_t* x0, uint32_t* x1, uint32_t* mrc, uint32_t nsym)
{
    const uint32_t sidx = blockIdx.x * 4 + (threadIdx.x >> 6); const int i = threadIdx.x & 63;
    if (sidx >= nsym) return;
    const uint32_t* c = ch + (size_t)(frame_index ? frame_index[sidx] : 0u) * 128;
    cpx a, b;
    const cpx m = siso_comp_mrc(unpack(y0[(size_t)sidx * 64 + i]), unpack(c[i]), unpack(y1[(size_t)sidx * 64 + i]), unpack(c[64 + i]), a, b);
    if (x0) x0[(size_t)sidx * 64 + i] = pack(a);
    if (x1) x1[(size_t)sidx * 64 + i] = pack(b);
    if (mrc) mrc[(size_t)sidx * 64 + i] = pack(m);
}

// ---- T11nSigDemap (demapper11n.hpp:6-87): three symbols per frame, L-SIG on I, HT-SIG 1/2 on Q; one wave per symbol, lane < 48 = carrier
__global__ void __launch_bounds__(256) k_sig_demap11n_batch(const uint32_t* sym, uint8_t* soft, uint32_t nframes)
{
    __shared__ uint8_t s_lut[6][256];
    fill_demap_luts(s_lut);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6);                  // symbol number = 3 * frame + s
    if (g >= nframes * 3u || lane >= 48) return;
    soft[(size_t)g * 48 + lane] = sig_demap_soft(unpack(sym[(size_t)g * 64 + carrier_bin48(lane)]), (int)(g % 3u), s_lut);
}

// ---- T11aDeinterleaveBPSK x3 -> T11nViterbiSig (viterbi.hpp:51-99) -> T11nSigParser (PHY_11n.hpp:432-513): one wave per frame,
// lane = trellis state (Viterbi_sig11, viterbicore.h:36-261, over NB = 24 and NB = 48 steps)
__global__ void __launch_bounds__(256) k_sig_decode11n_batch(const uint8_t* soft, uint32_t* rec, uint32_t nframes)
{
    __shared__ uint8_t s_soft[4][144];
    __shared__ uint64_t s_dec[4][50];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t f = blockIdx.x * 4 + w;
    if (f >= nframes) return;                                                // whole waves leave; no block-wide barrier below
    for (int k = lane; k < 144; k += 64) { const int s3 = k / 48, kk = k - 48 * s3; s_soft[w][k] = soft[(size_t)f * 144 + 48 * s3 + sig_deint_index(kk)]; }
    __builtin_amdgcn_s_waitcnt(0); __builtin_amdgcn_wave_barrier();
    const uint32_t lsig = (uint32_t)(viterbi_sig_wave<24>(s_soft[w], s_dec[w], lane) >> 6);
    __builtin_amdgcn_wave_barrier();
    const uint64_t ht = viterbi_sig_wave<48>(s_soft[w] + 48, s_dec[w], lane) >> 6;
    if (lane != 0) return;
    // the record: what the parser had extracted when it stopped (the reference's gate: 8 <= MCS < 11, at most 1500 bytes)
    const SigFront P = sig_parse_front(lsig, ht);
    uint32_t fl[9] = { 0, P.rate_kbps, P.lsig_len, 0, 0, 0, 0, 0, 0 };
    bool ok = false;
    do {
        if (!P.ok) break;
        fl[3] = P.mcs;
        if (fl[3] < 8 || fl[3] >= 11) break;
        fl[4] = P.ht_len;
        if (fl[4] > 1500) break;
        fl[5] = code_rate11n(fl[3]);                                         // CR_34 : CR_12
        const uint32_t nd = data_bits11n(104u * nbpsc11n(fl[3]), fl[5]);     // DOT11N_RATE_PARAMS[8..10].ndbps
        fl[6] = fl[7] = (fl[4] * 8 + 22 + nd - 1) / nd + 4;
        fl[2] = fl[4]; fl[8] = 3;                                            // frame_length = ht_frame_length; SYMBOL_HT_STF
        ok = true;
    } while (0);
    if (!ok) fl[0] = E_PLCP_HEADER_FAIL;
    uint32_t* o = rec + (size_t)f * 12;
    for (int i = 0; i < 9; i++) o[i] = fl[i];
    o[9] = lsig & 0xFFFFFF; o[10] = (uint32_t)ht; o[11] = (uint32_t)(ht >> 32);
}

// TFreqEstimator_11n (freqoffset_11n.hpp:42-160): one wave per frame, lane = sample of the first L-LTF half, both RX chains
__global__ void __launch_bounds__(256) k_cfo_est11n_batch(const uint32_t* l0, const uint32_t* l1, short* state, uint32_t nframes, const short* atan_tab)
{
    const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6); const int i = threadIdx.x & 63;
    if (f >= nframes) return;
    const int delta = cfo_est11n(atan_tab, unpack(l0[(size_t)f * 128 + i]), unpack(l0[(size_t)f * 128 + 64 + i]), unpack(l1[(size_t)f * 128 + i]),
                                 unpack(l1[(size_t)f * 128 + 64 + i]));
    if (i < 8) {
        short* st = state + (size_t)f * 24;
        st[i] = (short)(i * delta); st[8 + i] = (short)(delta << 3); st[16 + i] = 0;
    }
}

// TFreqComp_11n (freqoffset_11n.hpp:162-280): frame f owns nbursts[f] bursts of 8 samples from sample first[f] of both chains;
// one thread per sample; the running phase is delta0 + burst * step - theta in wrapping int16
__global__ void __launch_bounds__(256) k_freq_comp11n_batch(const uint32_t* in0, const uint32_t* in1, uint32_t* out0, uint32_t* out1, const uint32_t* first,
                                                            const uint32_t* nbursts, const short* state, const uint32_t* sincos)
{
    const uint32_t f = blockIdx.y, nb = nbursts[f];
    const short* st = state + (size_t)f * 24;
    for (uint32_t m = blockIdx.x * 256 + threadIdx.x; m < nb * 8; m += gridDim.x * 256) {
        const int k = m & 7, b = m >> 3;
        const int ph = (int)(short)(st[k] + (short)(b * st[8 + k]) - st[16 + k]);
        const cpx cof = unpack(sincos[(unsigned)ph & 0xFFFFu]);
        const size_t at = (size_t)first[f] + m;
        out0[at] = pack(freq_comp11n(unpack(in0[at]), cof)); out1[at] = pack(freq_comp11n(unpack(in1[at]), cof));
    }
}
__global__ void k_freq_comp11n_advance(const uint32_t* nbursts, short* state, uint32_t nframes)       // vfo_delta_i += nbursts * vfo_step_i
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nframes * 8) return;
    short* st = state + (size_t)(t >> 3) * 24; const int k = t & 7;
    st[k] = (short)(st[k] + (short)(nbursts[t >> 3] * st[8 + k]));
}

// TPilotTrack_11n (pilot_11n.hpp:84-141): one wave per frame, 64 symbols per pass: per-symbol mean pilot phase, then a wrapping prefix sum
__global__ void __launch_bounds__(256) k_pilot_track11n_batch(const uint32_t* x0, const uint32_t* x1, const uint32_t* first, const uint32_t* nsym,
                                                              short* state, short* theta_out, uint32_t nframes, const short* atan_tab)
{
    const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6); const int lane = threadIdx.x & 63;
    if (f >= nframes) return;
    short* st = state + (size_t)f * 24;
    int base[8];
#pragma unroll
    for (int k = 0; k < 8; k++) base[k] = st[16 + k];
    const uint32_t n = nsym[f], s0 = first[f];
    int run = 0;                                                           // sum of the increments so far (the same for all 8 entries)
    for (uint32_t p = 0; p < n; p += 64) {
        const uint32_t s = p + lane;
        int inc = 0;
        if (s < n) {
            int t[2];
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const uint32_t* x = (c ? x1 : x0) + (size_t)(s0 + s) * 64;
                const cpx a = unpack(x[64 - 21]), b = unpack(x[64 - 7]), d = unpack(x[7]), e = unpack(x[21]);
                t[c] = (int)(short)((dsp_atan16(atan_tab, a.re, a.im) + dsp_atan16(atan_tab, b.re, b.im) + dsp_atan16(atan_tab, d.re,
                        d.im) + dsp_atan16(atan_tab, e.re, e.im)) >> 2);
            }
            inc = (int)(short)((t[0] + t[1]) >> 1);
        }
        int pre = inc;                                                     // inclusive prefix sum over the pass (wrapping in the end)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(pre, d); if (lane >= d) pre += v; }
        if (theta_out && s < n)
#pragma unroll
            for (int k = 0; k < 8; k++) theta_out[(size_t)(s0 + s) * 8 + k] = (short)(base[k] + run + pre);
        run += __shfl(pre, 63);
    }
    if (lane < 8) st[16 + lane] = (short)(base[lane] + run);
}

// ------------------------------------------------------------------------------------------------
// The bricks that complete CreateDemodGraph11n (fb11ndemod_config.hpp:166-264) as stages: TCCA11n, T11nDataSymbol, TStreamJoin + TStreamConcat, and the tail that the
// 802.11a graph shares, T11aDesc -> TBB11aFrameSink.
//
// ---- TCCA11n (cca_11n.hpp:25-170) over MimoAutoCorr (autocorr.hpp:5-147): one wave per stream, four streams per workgroup, tiles of 64 bursts (256 samples).
// Phase 1, position-parallel: lane l holds samples l, 64 + l, 128 + l, 192 + l of the tile.  The brick's wrapping running sums are, from a constructed brick, the sums of
// the last 32 products mod 2^32, so a sample's change of a sum is (product at i) - (product at i - 32), both functions of the raw samples i - 64 .. i that the tile and
// the record's 64-sample history hold in LDS; an inclusive wave scan of the changes on top of the sums carried from the sample before gives every sample's six sums.
// acorr and energy follow per lane; the energy 64 samples earlier is a plain delay for the whole call (the ring slips against the samples only at a detection, which ends
// the stream's consumption), so it is read from the tile itself, or from the record's ring laid out in delay order in front of it.  eb is only ever compared with 5:
// energy / den > 5  <=>  den <= energy / 6 for den >= 1, one division by a constant instead of a 64-bit division per sample.
// Phase 2, serial: two ballots per 64 samples (rise: eb > 5 && acorr > energy >> 1; fall: acorr < energy >> 3) and the three counters.  The walk jumps from event to event
// -- the next rise bit or the burst end at which sense_count reaches 84; the next fall bit or the sample that takes peak_count past 160 -- and never touches a sample.
// Every value of the walk is wave-uniform.  Domain: the records reachable from a constructed brick (peak_found set implies sense_count 0).
constexpr int kCcaWords = 264;                 // sora_cca11n_state: 8 words, the ring as 64 word pairs, 2 x 64 history samples
constexpr int kCcaTile = 256;                  // samples per tile
constexpr uint32_t kCcaMaxSense = 84, kCcaMaxBursts = 0x3FFFFFFFu;
struct CcaLds { uint32_t x[2][64 + kCcaTile]; long long e[64 + kCcaTile]; };      // index k = the sample 64 - k in front of the tile's first / sample k - 64 of the tile

__device__ __forceinline__ bool cca_eb_gt5(long long energy, long long his)       // energy >= 0: a square.  LLONG_MAX + 1 wraps to a negative denominator: eb <= 0
{
    const long long den = (long long)((unsigned long long)his + 1ull);
    if (den > 0) return (unsigned long long)den <= (unsigned long long)energy / 6ull;
    return den == 0 && energy > 5;                                                 // (the compiled reference divides by 1 there; not reachable: energies are >= 0)
}
__device__ __forceinline__ uint32_t cca_next_bit(const uint64_t (&m)[4], uint32_t pos, uint32_t none)
{
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        if (q < (pos >> 6)) continue;
        uint64_t w = m[q];
        if (q == (pos >> 6)) w &= ~0ull << (pos & 63u);
        if (w) return 64u * q + (uint32_t)__builtin_ctzll(w);
    }
    return none;
}

__global__ void __launch_bounds__(256) k_cca11n(const uint32_t* __restrict__ in0, const uint32_t* __restrict__ in1, const uint32_t* __restrict__ first, const uint32_t* __restrict__ n,
        uint32_t* __restrict__ state, uint32_t* __restrict__ used_out, uint32_t nstreams, uint32_t flags)
{
    __shared__ CcaLds s_w[4];
    const int lane = threadIdx.x & 63;
    const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= nstreams) return;                                               // whole waves leave; no block-wide barrier below
    CcaLds& W = s_w[threadIdx.x >> 6];
    uint32_t* st = state + (size_t)kCcaWords * f;
    // words: 0 cca_state, 1 error_code, 2 cca_pwr_reading, 3 sense_count, 4 peak_found, 5 peak_count, 6 his_index, 7 timeouts, 8.. ring, 136.. / 200.. history
    uint32_t cca_state = (uint32_t)uni((int)st[0]), err = (uint32_t)uni((int)st[1]), reading = (uint32_t)uni((int)st[2]), sc = (uint32_t)uni((int)st[3]);
    uint32_t pf = (uint32_t)uni((int)st[4]) ? 1u : 0u, pc = (uint32_t)uni((int)st[5]), timeouts = (uint32_t)uni((int)st[7]);
    const uint32_t his0 = (uint32_t)uni((int)st[6]) & 63u;
    const uint32_t nb = min((uint32_t)uni((int)n[f]), kCcaMaxBursts);
    if (cca_state != 0 || err != 0 || nb == 0) { if (lane == 0) used_out[f] = 0; return; }
    const uint32_t total = 4u * nb;
    const uint32_t* p[2] = { in0 + (size_t)first[f], in1 + (size_t)first[f] };
    {
        const uint32_t r = (his0 + (uint32_t)lane) & 63u;
        W.e[lane] = (long long)(((unsigned long long)st[8 + 2 * r + 1] << 32) | st[8 + 2 * r]);
        W.x[0][lane] = st[136 + lane]; W.x[1][lane] = st[200 + lane];
    }
    wave_lds_sync();
    unsigned carry[6];                                                       // the six moving sums as they stand in front of the tile: re, im, energy per chain
#pragma unroll
    for (int r = 0; r < 2; r++) {
        int cr = 0, ci = 0, e = 0;
        if (lane < 32) { conj_mul32(unpack(W.x[r][32 + lane]), unpack(W.x[r][lane]), cr, ci); cr >>= 5; ci >>= 5; e = sqnorm(unpack(W.x[r][32 + lane])) >> 5; }
        unsigned v[3] = { (unsigned)cr, (unsigned)ci, (unsigned)e };
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] += (unsigned)__shfl_xor((int)v[c], o);
#pragma unroll
        for (int c = 0; c < 3; c++) carry[3 * r + c] = v[c];
    }
    uint32_t t0 = 0, used = 0, recorded = 0;
    bool done = false;
    const bool rearm = (flags & SORA_CCA11N_REARM) != 0;
    for (;;) {
        const uint32_t nv = min((uint32_t)kCcaTile, total - t0);             // a whole number of bursts
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t i = 64u * q + lane;
            W.x[0][64 + i] = i < nv ? p[0][(size_t)t0 + i] : 0u; W.x[1][64 + i] = i < nv ? p[1][(size_t)t0 + i] : 0u;
        }
        wave_lds_sync();
        uint64_t rise[4], fall[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t i = 64u * q + lane, k = 64u + i;
            unsigned d[6];
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const cpx a = unpack(W.x[r][k]), b = unpack(W.x[r][k - 32]), c = unpack(W.x[r][k - 64]);
                int cr, ci, qr, qi;
                conj_mul32(a, b, cr, ci); conj_mul32(b, c, qr, qi);
                d[3 * r] = (unsigned)(cr >> 5) - (unsigned)(qr >> 5); d[3 * r + 1] = (unsigned)(ci >> 5) - (unsigned)(qi >> 5);
                d[3 * r + 2] = (unsigned)(sqnorm(a) >> 5) - (unsigned)(sqnorm(b) >> 5);
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1)
#pragma unroll
                for (int c = 0; c < 6; c++) { const unsigned t = (unsigned)__shfl_up((int)d[c], o); if (lane >= o) d[c] += t; }
#pragma unroll
            for (int c = 0; c < 6; c++) { d[c] += carry[c]; carry[c] = (unsigned)__shfl((int)d[c], 63); }
            const int re = (int)((unsigned)((int)d[0] >> 1) + (unsigned)((int)d[3] >> 1)), im = (int)((unsigned)((int)d[1] >> 1) + (unsigned)((int)d[4] >> 1));
            const int v = (int)((unsigned)((int)d[2] >> 1) + (unsigned)((int)d[5] >> 1));
            const long long acorr = (long long)((unsigned long long)((long long)re * re) + (unsigned long long)((long long)im * im));
            const long long energy = (long long)v * v;
            W.e[k] = energy;
            const long long his = W.e[i];                                     // 64 samples earlier: the ring's entry for this sample (written a pass ago at the latest)
            const bool valid = i < nv;
            rise[q] = __ballot(valid && cca_eb_gt5(energy, his) && acorr > (energy >> 1));
            fall[q] = __ballot(valid && acorr < (energy >> 3));
            wave_lds_sync();
        }
        // ---- the decision walk over the tile's two bit masks
        uint32_t pos = 0;
        while (pos < nv) {
            if (!pf) {
                const uint32_t nx = cca_next_bit(rise, pos, nv);
                const uint32_t need = sc >= kCcaMaxSense ? 0u : kCcaMaxSense - sc;
                const uint32_t e = (pos + (need ? need - 1u : 0u)) | 3u;      // the burst end at which sense_count has reached 84, were no rise in between
                if (e < nx) {                                                // carrier-sense time-out behind burst (t0 + e) / 4
                    used = (t0 + e) / 4u + 1u; recorded = t0 + e + 1u;
                    sc += e + 1u - pos; pc = 0;
                    if (!rearm) { err = (uint32_t)SORA_E_CS_TIMEOUT; done = true; break; }
                    sc = 0; pf = 0; pc = 0; timeouts++;                      // _reset(), as RxThread does after the event
                    pos = e + 1u;
                    continue;
                }
                if (nx > pos) { sc += nx - pos; pc = 0; }
                pos = nx;
                if (pos < nv) { sc = 0; pc++; pf = 1; pos++; }
            } else {
                const uint32_t nx = cca_next_bit(fall, pos, nv);
                const uint32_t r = pos + (pc >= 160u ? 0u : 160u - pc);       // the sample that takes peak_count past 160
                if (r < nx) { pf = 0; pc = 0; pos = r + 1u; continue; }       // too many peaks
                pc += nx - pos; pos = nx;
                if (pos < nv) {
                    const bool good = pc > 96u && pc < 160u;
                    pf = 0; pc = 0;
                    if (good) {                                              // OnPowerDetected: the rest of the burst is consumed, but neither looked at nor recorded
                        reading = (uint32_t)((unsigned long long)W.e[pos] >> 32);
                        cca_state = 1; used = (t0 + pos) / 4u + 1u; recorded = t0 + pos; done = true;
                        break;
                    }
                    pos++;                                                   // a fake plateau
                }
            }
        }
        if (done) break;
        used = (t0 + nv) / 4u; recorded = t0 + nv;
        if (nv < (uint32_t)kCcaTile || t0 + kCcaTile >= total) break;
        {                                                                    // the last 64 samples and energies move in front of the next tile
            const uint32_t x0 = W.x[0][kCcaTile + lane], x1 = W.x[1][kCcaTile + lane]; const long long e = W.e[kCcaTile + lane];
            wave_lds_sync();
            W.x[0][lane] = x0; W.x[1][lane] = x1; W.e[lane] = e;
            wave_lds_sync();
        }
        t0 += kCcaTile;
    }
    // ---- the record as the brick would hold it: ring entry (his_index + i) mod 64 = the energy of recorded sample i, history = the last 64 samples consumed
    {
        const long long e = W.e[recorded - t0 + lane];
        const uint32_t r = (his0 + recorded + (uint32_t)lane) & 63u, c = 4u * used - t0 + lane;
        const uint32_t h0 = W.x[0][c], h1 = W.x[1][c];
        st[8 + 2 * r] = (uint32_t)(unsigned long long)e; st[8 + 2 * r + 1] = (uint32_t)((unsigned long long)e >> 32);
        st[136 + lane] = h0; st[200 + lane] = h1;
    }
    if (lane == 0) {
        st[0] = cca_state; st[1] = err; st[2] = reading; st[3] = sc; st[4] = pf; st[5] = pc; st[6] = (his0 + recorded) & 63u; st[7] = timeouts;
        used_out[f] = used;
    }
}

// ---- T11nDataSymbol (PHY_11n.hpp:288-356): the cyclic prefix of both chains dropped.  A thread moves four samples of both chains: one 16-byte load where the frame's
// first sample is 16-byte aligned (four 4-byte loads where it is not), one 16-byte store where the output buffers are.
__global__ void __launch_bounds__(256) k_data_symbol11n(const uint32_t* __restrict__ in0, const uint32_t* __restrict__ in1, uint32_t* __restrict__ out0, uint32_t* __restrict__ out1,
        const uint32_t* __restrict__ first, const uint32_t* __restrict__ nsym, const uint32_t* __restrict__ out_first)
{
    const uint32_t f = blockIdx.y, n = min(nsym[f], 1u << 27);
    const size_t src = first[f], dst = (size_t)out_first[f] * 64;
    const bool vin = (((uintptr_t)(in0 + src) | (uintptr_t)(in1 + src)) & 15) == 0, vout = (((uintptr_t)out0 | (uintptr_t)out1) & 15) == 0;
    for (uint32_t m = blockIdx.x * 256 + threadIdx.x; m < n * 16u; m += gridDim.x * 256) {
        const uint32_t k = m >> 4, j = m & 15u;
        const size_t a = src + (size_t)k * 80 + 16 + 4 * j, o = dst + (size_t)k * 64 + 4 * j;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const uint32_t* s = (c ? in1 : in0) + a; uint32_t* d = (c ? out1 : out0) + o;
            const uint4 v = vin ? *reinterpret_cast<const uint4*>(s) : uint4{ s[0], s[1], s[2], s[3] };
            if (vout) *reinterpret_cast<uint4*>(d) = v; else { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
        }
    }
}

// ---- TStreamJoin<2, 52 N_BPSC> -> TStreamConcat<2, s> (stdbrick.hpp:640-720): groups of s bytes, alternating spatial stream 0 and 1.  52 N_BPSC is a multiple of s for
// every modulation, so the symbols' borders fall on group borders and the whole call is ONE interleave of two byte streams: output byte B comes from byte
// s (B / 2s) + B mod s of stream (B / s) & 1.  A thread turns 48 bytes of each stream (three 16-byte loads each) into 96 output bytes (six 16-byte stores): 96 is a
// multiple of every group pair 2s.  Bytes behind the last whole chunk, and every byte where a buffer is not 16-byte aligned, go one by one.
template <int S>
__global__ void __launch_bounds__(256) k_stream_join11n(const uint8_t* __restrict__ s0, const uint8_t* __restrict__ s1, uint8_t* __restrict__ out, uint64_t total, uint64_t vec_chunks)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < vec_chunks) {
        uint32_t a[2][12], o[24];
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int w = 0; w < 3; w++) {
                const uint4 v = reinterpret_cast<const uint4*>((c ? s1 : s0) + t * 48)[w];
                a[c][4 * w] = v.x; a[c][4 * w + 1] = v.y; a[c][4 * w + 2] = v.z; a[c][4 * w + 3] = v.w;
            }
#pragma unroll
        for (int w = 0; w < 24; w++) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int B = 4 * w + b, src = S * (B / (2 * S)) + B % S, c = (B / S) & 1;
                v |= ((a[c][src >> 2] >> (8 * (src & 3))) & 0xFFu) << (8 * b);
            }
            o[w] = v;
        }
#pragma unroll
        for (int w = 0; w < 6; w++) reinterpret_cast<uint4*>(out + t * 96)[w] = uint4{ o[4 * w], o[4 * w + 1], o[4 * w + 2], o[4 * w + 3] };
        return;
    }
    const uint64_t tail = total - vec_chunks * 96;                            // the bytes behind the chunks, strided over the threads behind them
    const uint64_t nthreads = (uint64_t)gridDim.x * 256 - vec_chunks;
    for (uint64_t k = t - vec_chunks; k < tail; k += nthreads) {
        const uint64_t B = vec_chunks * 96 + k, src = (uint64_t)S * (B / (2 * S)) + B % S;
        out[B] = ((B / S) & 1) ? s1[src] : s0[src];
    }
}
template __global__ void k_stream_join11n<1>(const uint8_t*, const uint8_t*, uint8_t*, uint64_t, uint64_t);
template __global__ void k_stream_join11n<2>(const uint8_t*, const uint8_t*, uint8_t*, uint64_t, uint64_t);
template __global__ void k_stream_join11n<3>(const uint8_t*, const uint8_t*, uint8_t*, uint64_t, uint64_t);

// ---- T11aDesc (scramble.hpp:269-355): one wave per frame, the handle's table walk (dev_11n.h: desc11a_phase / desc11a_byte)
__global__ void __launch_bounds__(256) k_desc11a(const uint8_t* __restrict__ dec, const uint32_t* __restrict__ off, const uint32_t* __restrict__ len, uint8_t* __restrict__ out,
        const uint32_t* __restrict__ out_off, uint32_t n, Tables T)
{
    const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6); const int lane = threadIdx.x & 63;
    if (f >= n) return;
    const uint8_t* d = dec + off[f]; uint8_t* o = out + out_off[f];
    const uint32_t L = len[f];
    const unsigned phase = desc11a_phase(T, d);
    for (uint32_t i = lane; i < L; i += 64) o[i] = (uint8_t)desc11a_byte(T, phase, d, i);
}

// ---- TBB11aFrameSink (PHY_11a.hpp:609-700): one wave per frame; the frame into LDS (16 bytes per lane between the ragged ends), then the handle's parallel CRC-32
// (dev_11n.h: fcs_verdict, the form with two passes: 5120 bytes).  Below 4 bytes the brick never decides (frame_length - 4 is compared as ulong: every byte counts for the
// CRC and none for the FCS): the record is 0, 0.  Above kSinkBytes: lane 0, byte by byte.
constexpr uint32_t kSinkBytes = 4096;
__global__ void __launch_bounds__(256) k_frame_sink11a(const uint8_t* __restrict__ bytes, const uint32_t* __restrict__ off, const uint32_t* __restrict__ len, uint32_t* __restrict__ rec,
        uint32_t n, Tables T)
{
    __shared__ uint32_t s_crc[256];
    __shared__ uint32_t s_z[6 * 8 * 16];
    __shared__ uint4 s_bufs[4][kSinkBytes / 16 + 1];
    s_crc[threadIdx.x] = T.crc[threadIdx.x];
    for (int i = threadIdx.x; i < 6 * 8 * 16; i += 256) s_z[i] = T.crcz[i];
    __syncthreads();
    const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6); const int lane = threadIdx.x & 63;
    if (f >= n) return;
    const uint8_t* src = bytes + off[f];
    const uint32_t L = len[f] & 0xFFFFu;                                      // frame_length is a ushort
    uint32_t verdict = 0, fcs = 0;
    if (L >= 4 && L <= kSinkBytes) {
        const uint32_t mis = (uint32_t)((uintptr_t)src & 15);
        uint8_t* buf = reinterpret_cast<uint8_t*>(s_bufs[threadIdx.x >> 6]) + mis;      // LDS and HBM are 16-byte aligned at the same bytes
        const uint32_t head = min(L, (16u - mis) & 15u), body = (L - head) / 16u;
        if ((uint32_t)lane < head) buf[lane] = src[lane];
        for (uint32_t c = lane; c < body; c += 64) reinterpret_cast<uint4*>(buf + head)[c] = reinterpret_cast<const uint4*>(src + head)[c];
        for (uint32_t i = head + 16u * body + lane; i < L; i += 64) buf[i] = src[i];
        wave_lds_sync();
        verdict = fcs_verdict<true>(buf, L, s_crc, s_z, lane, fcs);
    } else if (L > kSinkBytes && lane == 0) {
        uint32_t crc = 0xFFFFFFFFu;
        for (uint32_t i = 0; i + 4 < L; i++) crc = (crc >> 8) ^ s_crc[(src[i] ^ crc) & 0xFF];
        fcs = (uint32_t)src[L - 4] | ((uint32_t)src[L - 3] << 8) | ((uint32_t)src[L - 2] << 16) | ((uint32_t)src[L - 1] << 24);
        verdict = ((~crc) == fcs) ? E_FRAME_OK : E_CRC32_FAIL;
    }
    if (lane == 0) { rec[2 * (size_t)f] = verdict; rec[2 * (size_t)f + 1] = fcs; }
}

}  // namespace sora

using namespace sora;

// ---- the stage entry points (host_stage.h: the prologue and helpers every stage shares)
int sora_hip_demap11n(const sora_complex16* d_in, uint8_t* d_soft, int n_bpsc, size_t n, void* stream)
{
    STAGE_ENTRY("sora_hip_demap11n", !d_in || !d_soft, n)
    STAGE_NBPSC("sora_hip_demap11n", n_bpsc)
    hipLaunchKernelGGL(k_demap11n_batch, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, u32(d_in), d_soft, n_bpsc, (uint32_t)n);
    return launch_result("k_demap11n_batch");
}

int sora_hip_deinterleave11n(const uint8_t* d_in, uint8_t* d_out, int n_bpsc, int spatial_stream, size_t n, void* stream)
{
    STAGE_ENTRY("sora_hip_deinterleave11n", !d_in || !d_out, n)
    STAGE_NBPSC("sora_hip_deinterleave11n", n_bpsc)
    if (spatial_stream < 0 || spatial_stream > 1) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_deinterleave11n: spatial_stream must be 0 or 1", 0);
    const uint64_t total = (uint64_t)n * 52 * n_bpsc;
    hipLaunchKernelGGL(k_deint11n_batch, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_in, d_out, n_bpsc, spatial_stream, (uint32_t)n);
    return launch_result("k_deint11n_batch");
}

int sora_hip_mimo_est11n(const sora_complex16* d_ltf0, const sora_complex16* d_ltf1, sora_complex16* d_h, sora_complex16* d_hinv, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_mimo_est11n", !d_ltf0 || !d_ltf1 || !d_h || !d_hinv, nframes)
    hipLaunchKernelGGL(k_mimo_est11n_batch, dim3((unsigned)((nframes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, u32(d_ltf0), u32(d_ltf1), u32(d_h), u32(d_hinv), (uint32_t)nframes);
    return launch_result("k_mimo_est11n_batch");
}

int sora_hip_mimo_comp11n(const sora_complex16* d_hinv, const uint32_t* d_frame_index, const sora_complex16* d_y0, const sora_complex16* d_y1,
                          sora_complex16* d_x0, sora_complex16* d_x1, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_mimo_comp11n", !d_hinv || !d_y0 || !d_y1 || !d_x0 || !d_x1, nsym)
    hipLaunchKernelGGL(k_mimo_comp11n_batch, dim3((unsigned)((nsym + 3) / 4)), dim3(256), 0, (hipStream_t)stream, u32(d_hinv), d_frame_index, u32(d_y0), u32(d_y1), u32(d_x0), u32(d_x1),
                       (uint32_t)nsym);
    return launch_result("k_mimo_comp11n_batch");
}

// ---- dsp_math tables (dsp_math.h:215-245): generated once per device with the C library, as the reference generates them at start-up
#include <cmath>
#include <mutex>
#include <vector>
// the two tables on the host (dsp_math.h:215-245)
void sora_internal_dsp_host_tables(std::vector<uint32_t>& sc, std::vector<short>& at)
{
    sc.resize(65536); at.resize(4097);
    for (unsigned i = 0; i < 65536; i++) {
        const double r = (double)i * 2.0 * M_PI / 65535.0;
        const short c = (short)(cos(r) * 32767.5), s = (short)(sin(r) * 32767.5);
        sc[i] = ((uint32_t)(uint16_t)c) | ((uint32_t)(uint16_t)s << 16);
    }
    for (int i = 0; i <= 4096; i++) at[i] = (short)(atan((double)i / 4096.0) / (M_PI / 4.0) * 8192);
}
namespace {
struct DspTables { uint32_t* sincos = nullptr; short* atan = nullptr; };
std::mutex g_dsp_mutex;
const DspTables* dsp_tables()
{
    static DspTables tabs[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    // handles may be created from different threads: built once per device, published whole
    std::lock_guard<std::mutex> lock(g_dsp_mutex);
    DspTables& T = tabs[dev];
    if (!T.sincos) {
        std::vector<uint32_t> sc; std::vector<short> at;
        sora_internal_dsp_host_tables(sc, at);
        if (sora_internal_pin_table("dsp_sincos", sc.data(), sc.size() * 4) != SORA_OK || sora_internal_pin_table("dsp_atan", at.data(), at.size() * 2) != SORA_OK) return nullptr;
        uint32_t* d_sc = nullptr; short* d_at = nullptr;
        if (hipMalloc((void**)&d_sc, sc.size() * 4) != hipSuccess || hipMalloc((void**)&d_at, at.size() * 2) != hipSuccess ||
            hipMemcpy(d_sc, sc.data(), sc.size() * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_at, at.data(), at.size() * 2, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d_sc); (void)hipFree(d_at);
            return nullptr;
        }
        T.atan = d_at; T.sincos = d_sc;                                         // (sincos last: it is what marks the entry as built)
    }
    return &T;
}
}  // namespace

int sora_internal_dsp_tables(const uint32_t** sincos, const short** atan)       // current device; used by k_rx11n.hip
{
    const DspTables* T = dsp_tables();
    if (!T) return SORA_ERR_HARDWARE_FAILED;
    *sincos = T->sincos; *atan = T->atan; return SORA_OK;
}

int sora_hip_cfo_est11n(const sora_complex16* d_lltf0, const sora_complex16* d_lltf1, int16_t* d_state, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_cfo_est11n", !d_lltf0 || !d_lltf1 || !d_state, nframes)
    const DspTables* T = dsp_tables(); if (!T) return sora_internal_fail(SORA_ERR_HARDWARE_FAILED, "dsp_math table upload failed", 0);
    hipLaunchKernelGGL(k_cfo_est11n_batch, dim3((unsigned)((nframes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, u32(d_lltf0), u32(d_lltf1), d_state, (uint32_t)nframes, T->atan);
    return launch_result("k_cfo_est11n_batch");
}

int sora_hip_freq_comp11n(const sora_complex16* d_in0, const sora_complex16* d_in1, sora_complex16* d_out0, sora_complex16* d_out1,
                          const uint32_t* d_first, const uint32_t* d_nbursts, int16_t* d_state, size_t nframes, size_t max_bursts, void* stream)
{
    STAGE_ENTRY("sora_hip_freq_comp11n", !d_in0 || !d_in1 || !d_out0 || !d_out1 || !d_first || !d_nbursts || !d_state, nframes)
    if (max_bursts == 0) return SORA_OK;
    if (nframes > 65535) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_freq_comp11n: at most 65535 frames per call", 0);
    const DspTables* T = dsp_tables(); if (!T) return sora_internal_fail(SORA_ERR_HARDWARE_FAILED, "dsp_math table upload failed", 0);
    const unsigned gx = (unsigned)((max_bursts * 8 + 255) / 256);
    hipLaunchKernelGGL(k_freq_comp11n_batch, dim3(gx < 64 ? gx : 64, (unsigned)nframes), dim3(256), 0, (hipStream_t)stream, u32(d_in0),
                       u32(d_in1), u32(d_out0), u32(d_out1), d_first, d_nbursts, d_state, T->sincos);
    hipLaunchKernelGGL(k_freq_comp11n_advance, dim3((unsigned)((nframes * 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_nbursts, d_state, (uint32_t)nframes);
    return launch_result("k_freq_comp11n_batch");
}

int sora_hip_pilot_track11n(const sora_complex16* d_x0, const sora_complex16* d_x1, const uint32_t* d_first, const uint32_t* d_nsym, int16_t* d_state,
                            int16_t* d_theta, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_pilot_track11n", !d_x0 || !d_x1 || !d_first || !d_nsym || !d_state, nframes)
    const DspTables* T = dsp_tables(); if (!T) return sora_internal_fail(SORA_ERR_HARDWARE_FAILED, "dsp_math table upload failed", 0);
    hipLaunchKernelGGL(k_pilot_track11n_batch, dim3((unsigned)((nframes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, u32(d_x0),
                       u32(d_x1), d_first, d_nsym, d_state, d_theta, (uint32_t)nframes, T->atan);
    return launch_result("k_pilot_track11n_batch");
}

int sora_hip_siso_est11n(const sora_complex16* d_lltf0, const sora_complex16* d_lltf1, sora_complex16* d_ch, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_siso_est11n", !d_lltf0 || !d_lltf1 || !d_ch, nframes)
    hipLaunchKernelGGL(k_siso_est11n_batch, dim3((unsigned)((nframes + 1) / 2)), dim3(256), 0, (hipStream_t)stream, u32(d_lltf0), u32(d_lltf1), u32(d_ch), (uint32_t)nframes);
    return launch_result("k_siso_est11n_batch");
}

int sora_hip_siso_comp11n(const sora_complex16* d_ch, const uint32_t* d_frame_index, const sora_complex16* d_y0, const sora_complex16* d_y1,
                          sora_complex16* d_x0, sora_complex16* d_x1, sora_complex16* d_mrc, size_t nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_siso_comp11n", !d_ch || !d_y0 || !d_y1 || !(d_x0 || d_x1 || d_mrc), nsym)
    hipLaunchKernelGGL(k_siso_comp11n_batch, dim3((unsigned)((nsym + 3) / 4)), dim3(256), 0, (hipStream_t)stream, u32(d_ch), d_frame_index, u32(d_y0), u32(d_y1), u32(d_x0),
                       u32(d_x1), u32(d_mrc), (uint32_t)nsym);
    return launch_result("k_siso_comp11n_batch");
}

int sora_hip_sig_demap11n(const sora_complex16* d_sym, uint8_t* d_soft, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_sig_demap11n", !d_sym || !d_soft, nframes)
    hipLaunchKernelGGL(k_sig_demap11n_batch, dim3((unsigned)((nframes * 3 + 3) / 4)), dim3(256), 0, (hipStream_t)stream, u32(d_sym), d_soft, (uint32_t)nframes);
    return launch_result("k_sig_demap11n_batch");
}

int sora_hip_sig_decode11n(const uint8_t* d_soft, uint32_t* d_rec, size_t nframes, void* stream)
{
    STAGE_ENTRY("sora_hip_sig_decode11n", !d_soft || !d_rec, nframes)
    hipLaunchKernelGGL(k_sig_decode11n_batch, dim3((unsigned)((nframes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_soft, d_rec, (uint32_t)nframes);
    return launch_result("k_sig_decode11n_batch");
}

// ---- the bricks that complete the receive graph (sora_hip_cca11n .. sora_hip_frame_sink11a)
static_assert(sizeof(sora_cca11n_state) == 4 * kCcaWords && sizeof(sora_sink11a_rec) == 8, "the 802.11n stage records are 32-bit words");

int sora_hip_cca11n(const sora_complex16* d_in0, const sora_complex16* d_in1, const uint32_t* d_first, const uint32_t* d_n, sora_cca11n_state* d_state, uint32_t* d_used,
                    size_t nstreams, size_t max_n, unsigned flags, void* stream)
{
    (void)max_n;                                                                 // (a wave per stream walks its own d_n[f])
    STAGE_ENTRY("sora_hip_cca11n", !d_in0 || !d_in1 || !d_first || !d_n || !d_state || !d_used, nstreams)
    if (flags & ~(unsigned)SORA_CCA11N_REARM) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_cca11n: unknown flag", 0);
    hipLaunchKernelGGL(k_cca11n, dim3((unsigned)((nstreams + 3) / 4)), dim3(256), 0, (hipStream_t)stream, u32(d_in0),
                       u32(d_in1), d_first, d_n, u32(d_state), d_used, (uint32_t)nstreams, (uint32_t)flags);
    return launch_result("k_cca11n");
}

int sora_hip_data_symbol11n(const sora_complex16* d_in0, const sora_complex16* d_in1, const uint32_t* d_first, const uint32_t* d_nsym, const uint32_t* d_out_first,
                            sora_complex16* d_out0, sora_complex16* d_out1, size_t nframes, size_t max_nsym, void* stream)
{
    STAGE_ENTRY("sora_hip_data_symbol11n", !d_in0 || !d_in1 || !d_first || !d_nsym || !d_out_first || !d_out0 || !d_out1, nframes)
    if (max_nsym == 0) return SORA_OK;
    if (nframes > 65535 || max_nsym > (1u << 27)) return sora_internal_fail(SORA_ERR_CAPACITY, "sora_hip_data_symbol11n: at most 65535 frames of 2^27 symbols per call", 0);
    const unsigned gx = (unsigned)((max_nsym * 16 + 255) / 256);
    hipLaunchKernelGGL(k_data_symbol11n, dim3(gx < 64 ? gx : 64, (unsigned)nframes), dim3(256), 0, (hipStream_t)stream, u32(d_in0),
                       u32(d_in1), u32(d_out0), u32(d_out1), d_first, d_nsym, d_out_first);
    return launch_result("k_data_symbol11n");
}

int sora_hip_stream_join11n(const uint8_t* d_s0, const uint8_t* d_s1, uint8_t* d_out, int n_bpsc, size_t n, void* stream)
{
    if (!d_s0 || !d_s1 || !d_out) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "sora_hip_stream_join11n: null pointer", 0);
    STAGE_NBPSC("sora_hip_stream_join11n", n_bpsc)                                // (before the prologue: refused for a count of 0 too)
    STAGE_ENTRY("sora_hip_stream_join11n", false, n)
    const uint64_t total = (uint64_t)n * 104 * n_bpsc;
    const uint64_t chunks = aligned16(d_s0, d_s1, d_out) ? total / 96 : 0, tail = total - chunks * 96;
    const uint64_t threads = chunks + (tail < 65536 ? tail : 65536);            // a thread per chunk, then the tail's bytes strided over up to 65536 more
    const unsigned grid = (unsigned)((threads + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    switch (n_bpsc) {
    case 4: hipLaunchKernelGGL(k_stream_join11n<2>, dim3(grid), dim3(256), 0, st, d_s0, d_s1, d_out, total, chunks); break;
    case 6: hipLaunchKernelGGL(k_stream_join11n<3>, dim3(grid), dim3(256), 0, st, d_s0, d_s1, d_out, total, chunks); break;
    default: hipLaunchKernelGGL(k_stream_join11n<1>, dim3(grid), dim3(256), 0, st, d_s0, d_s1, d_out, total, chunks); break;
    }
    return launch_result("k_stream_join11n");
}

int sora_hip_desc11a(const uint8_t* d_dec, const uint32_t* d_off, const uint32_t* d_len, uint8_t* d_out, const uint32_t* d_out_off, size_t n, void* stream)
{
    STAGE_ENTRY("sora_hip_desc11a", !d_dec || !d_off || !d_len || !d_out || !d_out_off, n)
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_desc11a, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_dec, d_off, d_len, d_out, d_out_off, (uint32_t)n, T);
    return launch_result("k_desc11a");
}

int sora_hip_frame_sink11a(const uint8_t* d_bytes, const uint32_t* d_off, const uint32_t* d_len, sora_sink11a_rec* d_rec, size_t n, void* stream)
{
    STAGE_ENTRY("sora_hip_frame_sink11a", !d_bytes || !d_off || !d_len || !d_rec, n)
    Tables T; if (const int rc = stage_tables(&T)) return rc;
    hipLaunchKernelGGL(k_frame_sink11a, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_bytes, d_off, d_len, u32(d_rec), (uint32_t)n, T);
    return launch_result("k_frame_sink11a");
}
