// dev_sym11a.h -- the pieces of the 802.11a data field's symbol chain (fb11ademod_config.hpp:200-222):
//   TFreqCompensation -> TFFT64 -> TChannelEqualization -> TPhaseCompensate -> TPilotTrack -> T11aDemap -> T11aDeinterleave -> soft stream
// Every form of the chain -- k_frame, k_sym_front / k_track_lds / k_sym_back, k_pipe, the fallback behind k_pipe (k_rx.hip) and the per-stage kernels
// (k_stage.hip) -- takes the reference's arithmetic from here and keeps only its own schedule, layout and hand-offs.
#pragma once
#include "kernels.h"
#include "dev_viterbi.h"
#include "dev_pilot11a.h"

namespace sora {

// ---- the frame's VitJob: its soft stream (one pre-scaled byte per value) and its decoded bytes sit at the frame's first symbol slot (rx_types.h)
__device__ __forceinline__ VitJob frame_vitjob(const FrameRow& r)
{
    VitJob J;
    J.valid = 1; J.soft_off = r.slot0 * (uint32_t)kSoftBytesPerSlot; J.nsoft = (uint32_t)r.nsym * 48u * r.nbpsc; J.length = r.length;
    J.dec_off = 0; J.out_off = r.slot0 * (uint32_t)kOutPerSlot; J.code_rate = r.code_rate; J.soft_bits = (uint32_t)kSoftScaled;
    return J;
}

// ---- pilot polarity: one bit of the sequence's four words is pilot_sgn (dev_pilot11a.h); here as the table a kernel indexes with a symbol count it holds in a register
static __device__ __constant__ PilotPolarity kPilotSgn = kPilotPolarity;
__device__ __forceinline__ int pilot_angle(int th, unsigned count) { return kPilotSgn.neg[count] ? w16(th + 0x8000) : th; }   // a pilot of polarity -1: + pi

// ---- TFreqCompensation and TChannelEqualization of one sample / one bin on packed COMPLEX16.  COEF: the frame's coefficient as stored (pcx: a caller with one
// symbol per frame -- turned into the packed product's operand pair where it is used, not held across the FFT) or already as that pair (PkTw: a caller that uses it
// for several symbols; pk_tw_mul takes either).  k_symfront_batch is why: converting its coefficients up front took it from 60 to 66 VGPRs, 8 waves per SIMD to 7.
template <typename COEF> __device__ __forceinline__ pcx sym_freq_comp(uint32_t raw, COEF fq) { return pk_cmul<15>(pk_sra(raw, 1), pk_tw_mul(fq)); }   // >>1, x FreqCoeffs (channel_11a.hpp:643-644)
template <typename COEF> __device__ __forceinline__ pcx sym_equalise(pcx y, COEF ch, int bin)                                                            // channel_11a.hpp:548-574
{
    return (bin >= 28 && bin < 36) ? 0u : pk_cmul<8>(y, pk_tw_mul(ch));
}
// ... and the two around TFFT64 for one quad of symbols, 16 lanes per symbol: group g's symbol from raw[] (its 64 samples behind the cyclic prefix, sample e + 16 m)
// x FreqCoeffs (e + 16 m), then x ChannelCoeffs (4 e + q); bins 4e .. 4e+3 out, one 16-byte store for the caller.  `sl` is the group's 64-word FFT staging, free
// again on return.
template <typename COEF>
__device__ __forceinline__ void sym_front_quad(const uint32_t raw[4], const COEF fq[4], const COEF ch[4], uint32_t* sl, int e, const Fft64TwPk& W, uint32_t o[4])
{
    pcx x[4];
#pragma unroll
    for (int m = 0; m < 4; m++) x[m] = sym_freq_comp(raw[m], fq[m]);
    fft64_core_pk(x, sl, e, W, wave_lds_sync);
    const unsigned rv = __brev((unsigned)e) >> 28;                               // bin 4e+q sits at slot bitrev6(4e+q) = bitrev4(e) + 16 bitrev2(q)
#pragma unroll
    for (int q = 0; q < 4; q++) o[q] = sym_equalise(sl[rv + 16u * ((q & 1) * 2 + (q >> 1))], ch[q], 4 * e + q);
    wave_lds_sync();
}

// ---- a wave's 16 consecutive symbol slots (four quads) and the frames that own them (slot_row[], written by k_scan)
constexpr int kSlotIters = 4;                                                    // quads of slots per wave
constexpr uint32_t kNoOwner = 0xFFFFFFFFu;                                       // preamble / silence
struct WaveSlots {
    uint32_t first;                                                              // the wave's first slot
    uint32_t my_own;                                                             // lane l < 16: the row that owns slot first + l
    unsigned long long owned;                                                    // bit l: slot first + l has an owner
    uint32_t row0;                                                               // the first owner
    bool one_frame;                                                              // the usual case: every owned slot of the wave belongs to ONE frame
    __device__ __forceinline__ uint32_t slot(int it, int g) const { return first + 4u * (uint32_t)it + (uint32_t)g; }
    __device__ __forceinline__ uint32_t owner(int it, int g) const { return (uint32_t)__shfl((int)my_own, 4 * it + g); }   // (all lanes call)
    __device__ __forceinline__ unsigned quad(int it) const { return (unsigned)(owned >> (4 * it)) & 0xFu; }               // owned slots of quad `it`, one bit per group
};
// wave w of workgroup `bid`.  owned == 0: none of its slots has an owner, nothing for the wave to do
__device__ __forceinline__ WaveSlots wave_slots(const RxArgs& A, uint32_t bid)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    WaveSlots S;
    S.first = (bid * 4u + (uint32_t)w) * (4u * kSlotIters);
    // lane l < 16 asks for slot first + l, the groups pick theirs up by cross-lane reads
    const uint32_t my_slot = S.first + (uint32_t)(lane & 15);
    S.my_own = (lane < 16 && my_slot < A.total_slots) ? A.slot_row[my_slot] : kNoOwner;
    S.owned = __ballot(S.my_own != kNoOwner);
    S.row0 = S.owned ? (uint32_t)__builtin_amdgcn_readlane((int)S.my_own, __builtin_ctzll(S.owned)) : kNoOwner;
    S.one_frame = __ballot(lane < 16 && S.my_own != kNoOwner && S.my_own != S.row0) == 0;
    return S;
}

// ---- TPilotTrack behind the four pilots' angles (pilot.hpp:213-232 -> freqoffset.hpp:28), global-table form: th1 .. th4 are the angles of carriers -21, -7, +7, +21
// with the polarity taken out (pilot_angle).  Returns the symbol's record { CFO_comp, SFO_comp before the symbol, its mean phase, its slope } and, for a symbol the
// frame has (act), advances the state.  How a form gets a frame's four angles into one lane -- quad broadcasts, readlane, four bins of a wave -- stays with the form.
// (k_track_lds / k_pipe run another exact formulation of the same step out of tables in LDS: track_step, k_rx.hip.)
__device__ __forceinline__ int4 track_advance(int th1, int th2, int th3, int th4, bool act, int& cfo_comp, int& sfo_comp, int& cfo_tr, int& sfo_tr)
{
    const int c0 = cfo_comp, s0 = sfo_comp;
    const int avg = w16((th1 + th2 + th3 + th4) / 4);
    const int del = w16(((th3 - th1) / 28 + (th4 - th2) / 28) >> 1);
    if (act) {
        cfo_tr = w16(cfo_tr + (avg >> 2)); sfo_tr = w16(sfo_tr + (del >> 2));
        cfo_comp = w16(cfo_comp + avg + cfo_tr); sfo_comp = w16(sfo_comp + del + sfo_tr);
    }
    return int4{ c0, s0, act ? avg : 0, act ? del : 0 };
}

// ---- TPhaseCompensate + TPilotTrack::_rotate + T11aDemap for one group's symbol (3 data carriers per lane, 16 lanes per symbol): the three bins v3
// (carriers e, e + 16, e + 32 in demap order) x CompCoeffs(rec.x, rec.y) x rotation(rec.z, rec.w) -> soft values in carrier order at `dst` (LDS).
__device__ __forceinline__ int4 track_rec4(TrackRec t) { return int4{ t.cfo_comp, t.sfo_comp, t.avg, t.del }; }
__device__ __forceinline__ void sym_back_demap(const Tables& T, const uint8_t* s_demap, const uint32_t v3[3], int4 rec, int nb, int e, uint8_t* dst)
{
    cpx c1[3], c2[3];
#pragma unroll
    for (int m = 0; m < 3; m++) {                                                // all six coefficient reads in flight together
        const int bin = carrier_bin48(e + 16 * m);
        const int c = bin < 32 ? bin : bin - 64;
        c1[m] = rot_coeff(T, w16(rec.x + c * rec.y));
        c2[m] = rot_coeff(T, w16(rec.z + c * rec.w));
    }
#pragma unroll
    for (int m = 0; m < 3; m++) {
        const int k = e + 16 * m;
        cpx v = mul_q15(unpack(v3[m]), c1[m]);
        v = mul_q15(v, c2[m]);
        int re = v.re >> 4, im = v.im >> 4;                                       // demap_limit<64> (demapper.h:141-151)
        re = min(max(re, -128), 127); im = min(max(im, -128), 127);
        const unsigned ur = (unsigned)re & 0xFF, ui = (unsigned)im & 0xFF;
        // DemapperCore::Demap<N_BPSC> (demapper.h:16-45): h = N_BPSC / 2 values per axis, value i of an axis out of step table 0, then 256 (16-QAM) or 512, 768
        // (64-QAM).  Written by depth, not as one list of stores per modulation: hipcc merges such lists' common first and last stores behind flag registers once
        // this is a function of its own, which cost k_frame 4 % of its time; this form is six straight stores behind three scalar branches.
        uint8_t* o = dst + k * nb;
        const int h = nb >> 1;
        o[0] = s_demap[ur];
        if (nb >= 2) {
            o[h] = s_demap[ui];
            if (nb >= 4) {
                const int t1 = nb == 4 ? 256 : 512;
                o[1] = s_demap[t1 + ur]; o[h + 1] = s_demap[t1 + ui];
                if (nb == 6) { o[2] = s_demap[768 + ur]; o[5] = s_demap[768 + ui]; }
            }
        }
    }
}

// ---- the demap step tables as a producer of the soft stream stages them in LDS: every entry (a soft value 0..7) doubled, so that what T11aDemap looks up and
// T11aDeinterleave gathers IS the stream's byte v << 1 (rx_types.h).  The table in HBM stays the reference's own (tests/test_table_pins.py).  256 threads.
__device__ __forceinline__ void demap_table_to_lds(const Tables& T, uint8_t* s_demap)
{
    reinterpret_cast<uint32_t*>(s_demap)[threadIdx.x] = (reinterpret_cast<const uint32_t*>(T.demap)[threadIdx.x] << 1) & 0xFEFEFEFEu;
}

// ---- T11aDeinterleave*: out[k] = in[j(k)] within a symbol, eight values -> eight bytes of the stream per lane (lane < N_CBPS / 8).
// The lane's source indices of output positions 8 lane .. 8 lane + 7 for modulation nb, two per register (0 for a lane that stores nothing)
__device__ __forceinline__ bool deint_packs(int nb, int lane) { return 8 * lane < 48 * nb; }
__device__ __forceinline__ void deint_map_words(const Tables& T, int nb, int lane, uint32_t mp[4])
{
    const uint16_t* map = T.deint + (nb == 1 ? 0 : nb == 2 ? 1 : nb == 4 ? 2 : 3) * 288;
    const bool packs = deint_packs(nb, lane);
#pragma unroll
    for (int t = 0; t < 4; t++) mp[t] = packs ? (uint32_t)map[8 * lane + 2 * t] | ((uint32_t)map[8 * lane + 2 * t + 1] << 16) : 0u;
}
// ... and the lane's eight bytes of one symbol, gathered out of its (doubled) soft values in carrier order (LDS): values 8 lane .. 8 lane + 3, then + 4 .. + 7
__device__ __forceinline__ uint2 deint_gather8(const uint8_t* src, const uint32_t mp[4])
{
    uint32_t v[8];
#pragma unroll
    for (int t = 0; t < 4; t++) { v[2 * t] = src[mp[t] & 0xFFFFu]; v[2 * t + 1] = src[mp[t] >> 16]; }
    return uint2{ v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24), v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24) };
}
// ... as one 8-byte store: bytes 8 lane .. 8 lane + 7 of the symbol at `sym` (8-byte aligned: a slot is 288 bytes, a symbol 48 N_BPSC)
__device__ __forceinline__ void soft8_store(uint8_t* sym, uint32_t lane, uint2 b) { reinterpret_cast<uint2*>(sym)[lane] = b; }

}  // namespace sora
