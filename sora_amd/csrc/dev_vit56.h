// dev_vit56.h -- the forward pass of the K=7 decoder at code rate 5/6 (SORA_CR_56, include/sora_hip.h) in the 64-lanes-per-pair layout:
// VitForward (dev_viterbi.h) restated for a puncture pattern that does not divide the 24-step row.  Everything the existing kernels are made of is used as it
// stands -- acs_step, the ring and its geometry, bank_word, viterbi_trace, the byte cursor -- and nothing in dev_viterbi.h changes; what is stated here is what differs:
//
//   the pattern   A puncture group is 6 soft values and 5 trellis steps of kinds (A,B) (A) (B) (A) (B): the three kinds acs_step has.  The kind of the step at
//                 t mod 24 depends on the row, so it cannot be baked into VitLane::MX as Puncture<CR>::which_of does: MX holds the A masks for every t, and a
//                 B-only step is acs_step<1> (one operand, K = 7) fed b ^ MD[t mod 6], MD = ma ^ mb of the phase -- (b ^ MD) ^ MX = b ^ (B mask, complemented and
//                 marked exactly where MX is).  One xor more per B-only step.
//   the loop      The pattern and the row repeat together every 120 steps = 24 groups = 144 soft values.  That period is the loop body, straight-line, every t mod 24
//                 a constant: six CHUNKS of 20 steps / 4 groups / 24 values, each handed over through the wave's operand table in LDS as VitForward does it
//                 (lane k < 32 fetches value k of frame A, lane 32 + k of frame B, two chunks ahead; six broadcast ds_read_b128 give every lane the 24 operand
//                 dwords).  Rows end inside chunks and inside groups: the ring position advances in front of the step at t mod 24 == 0, so that the schedule check
//                 behind a group always sees the row of the step just taken.
//   the rule      Normalisation follows every step whose index is a multiple of 8, also inside a group (the model's one changed rule): that is the step that banks a
//                 block and clears marks and guard, so the subtraction is the same single VOP2 on clean fields.  Per 8-step block a path's metric grows by at most
//                 2 x 14 + 6 x 7 = 70 units: it passes a multiple of 128 at most once per block, which is what acs_step's guard bit needs.
//   the schedule  cnt / look / remain are VitForward::check's expressions, examined after every group: remain and the final look reach 4.  A window's walk starts at
//                 tr <= ob + WIN + LOOK + 6 + 4 = ob + 238 and ends at block ob / 8: blocks ob / 8 .. (ob + 237) >> 3 = ob / 8 + 29, 30 blocks <= kMaxWalk = 31 --
//                 RingGeom<192, 36> holds as it stands (the static_assert below states it for any WIN / LOOK).  A frame's last walk starts below ob + 239 as well.
//   the stream    One raw byte per soft value, its low three bits; every fetch is a byte load clamped to min(the stream's last value, the caller's span - 1): nothing
//                 is read behind either, and a half whose frame has ended keeps stepping on its last well-formed value.  A side whose stream runs out in front of
//                 its last trace-back is done there (the model's loop ends with its soft values; VitForward lets such a side run on with the longer one).
#pragma once
#include "dev_viterbi.h"

namespace sora {

template <int WIN, int LOOK>
struct VitForward56 {
    using RG = RingGeom<WIN, LOOK>;
    static constexpr int P = RG::P;
    static constexpr int GB = 6, GS = 5;                                        // soft values / trellis steps per puncture group
    static constexpr int CS = 20, CW = 24, NCHUNK = 6;                          // steps / operands per chunk, chunks per 120-step period
    static_assert(WIN % 8 == 0 && (WIN + LOOK + 6 + (GS - 1) - 1) / 8 + 1 <= RG::kMaxWalk, "a walk from ob + WIN + LOOK + 6 + 4 down to block ob / 8 fits the ring's walk");
    struct Chunk { uint32_t v[CW]; };

    VitLane V;
    unsigned MD[6];                                                             // ma ^ mb per t mod 6: turns MX's A mask into the B mask
    VitSide A, B;
    uint32_t nsteps;                                                            // of the longer side
    uint32_t tr, ob, next_thr;
    SoftCursor<kSoftScaled, CW> cur;                                            // (its fetch: one byte at a clamped offset; the bytes here are raw, see put)
    const uint8_t* soft_base;
    uint16_t *ops, *my_op;

    // span: bytes of the soft buffer the jobs address (>= 1)
    __device__ __forceinline__ void init(const VitSide& A_, const VitSide& B_, const uint8_t* __restrict__ soft_base_, uint32_t span, uint16_t* ring, uint16_t* ops_)
    {
        const unsigned lane = threadIdx.x & 63;
        A = A_; B = B_;
        nsteps = max(A.nsteps, B.nsteps);
        const VitSide& M = lane >= 32u && !B.done ? B : A;
        const uint32_t my_k = lane & 31u;
        const unsigned vl = lane_map(lane);
        V.U = vl == 0 ? 0u : 0x18u * kFld;                                      // ALL_INIT0 / ALL_INIT = 0x00 / 0x30 (viterbilut.h:22-30)
        V.ring = ring; V.rowpos = (unsigned)(P - 3) * 64u;                      // the first step's begin_row makes it 0
        V.sidx[0] = __brev(rol6(vl, 2)) >> 26; V.sidx[1] = __brev(rol6(vl, 4)) >> 26; V.sidx[2] = __brev(vl) >> 26;
#pragma unroll
        for (int t = 0; t < 24; t++) {
            const int ph = t % 6, k = t % 8;
            const unsigned n = rol6(vl, ph + 1);
            const bool own1 = ph >= 2 && ((vl >> (5 - ph)) & 1);
            const unsigned ma = (__popc(n & 0155) & 1) ? 7u * kFld : 0u, mb = (__popc(n & 0117) & 1) ? 7u * kFld : 0u;
            V.MX[t] = own1 ? ((ma ^ (7u * kFld)) | (kOne << k)) : ma;
            if (t < 6) { V.MY[t] = own1 ? (mb ^ (7u * kFld)) : mb; MD[t] = ma ^ mb; }
        }
        tr = 0; ob = 0;
        cur.init(M.soft_off, my_k, M.last);
        cur.lim = min(cur.lim, span - 1u);
        soft_base = soft_base_; ops = ops_;
        my_op = ops + 2u * my_k + (lane >> 5);
    }
    __device__ __forceinline__ bool going() const { return tr < nsteps && !(A.done && B.done); }
    __device__ __forceinline__ void normalize() { V.U = V.U - dpp_pkmin_wave(V.U); }
    __device__ __forceinline__ void begin_row() { V.rowpos = V.rowpos + 3 * 64 == (unsigned)P * 64 ? 0u : V.rowpos + 3 * 64; }

    __device__ __forceinline__ uint32_t fetch(uint32_t c) const { return cur.fetch(soft_base, c).w; }
    __device__ __forceinline__ Chunk unpack(uint32_t raw)
    {
        *my_op = (uint16_t)((raw & 7u) << 9);                                   // the low three bits as the 16-bit metric field u << 9
        lds_fence();
        Chunk K;
#pragma unroll
        for (int i = 0; i < CW / 4; i++) {
            const uint4 x = reinterpret_cast<const uint4*>(ops)[i];
            K.v[4 * i] = x.x; K.v[4 * i + 1] = x.y; K.v[4 * i + 2] = x.z; K.v[4 * i + 3] = x.w;
        }
        lds_fence();
        return K;
    }

    // step S of the 120-step period; WHICH as acs_step's
    template <int WHICH, int S> __device__ __forceinline__ void step(unsigned x, unsigned y)
    {
        constexpr int t24 = S % 24;
        if constexpr (t24 == 0) begin_row();
        if constexpr (WHICH == 2) acs_step<1, P>(V, t24, x ^ MD[t24 % 6], 0);
        else acs_step<WHICH, P>(V, t24, x, y);
        if constexpr (t24 % 8 == 7) normalize();
    }
    // the puncture group that starts at step S of the period (a multiple of 5): A1 B1 A2 B3 A4 B5
    template <int S> __device__ __forceinline__ void group(const Chunk& K)
    {
        constexpr int k0 = S % CS / GS * GB;
        step<0, S>(K.v[k0], K.v[k0 + 1]);
        step<1, S + 1>(K.v[k0 + 2], 0);
        step<2, S + 2>(K.v[k0 + 3], 0);
        step<1, S + 3>(K.v[k0 + 4], 0);
        step<2, S + 4>(K.v[k0 + 5], 0);
    }

    __device__ __forceinline__ uint32_t next_event() const
    {
        uint32_t t = ob + (uint32_t)(WIN + LOOK + 6);
        if (!A.done) t = min(t, min(A.tr_end, A.nsteps));
        if (!B.done) t = min(t, min(B.tr_end, B.nsteps));
        return t;
    }
    // the trace-back schedule behind a group (VitForward::check); T24 = t mod 24 of the group's last step
    template <int T24> __device__ __forceinline__ void check()
    {
        if (tr >= next_thr) {
            constexpr int k = T24 % 8;
            const uint32_t pos = V.rowpos + (uint32_t)(T24 / 8) * 64u;          // ring position (x 64) of block (tr - 1) >> 3
            unsigned lastA, lastB;
            if (k == 7) { const unsigned w = V.ring[pos + V.sidx[T24 / 8]]; lastA = (w >> 7) & 1u; lastB = (w >> 15) & 1u; }
            else { lastA = (V.U >> k) & 1u; lastB = (V.U >> (17 + k)) & 1u; }
            const unsigned mA = ((V.U & 0xFFFFu) >> 9 << 1) | lastA, mB = (V.U >> 25 << 1) | lastB;
            const bool partial = tr >= ob + (uint32_t)(WIN + LOOK + 6);
            uint32_t cntA = 0, cntB = 0;
            if (!A.done) {
                if (tr >= A.tr_end) { cntA = A.tr_end - ob - 6; A.done = true; }
                else if (partial) cntA = WIN;
            }
            if (!B.done) {
                if (tr >= B.tr_end) { cntB = B.tr_end - ob - 6; B.done = true; }
                else if (partial) cntB = WIN;
            }
            if (cntA | cntB) viterbi_trace<RG::kMaxWalk>(V.U, V.ring, tr, ob, mA, mB, cntA, cntB, A.out, B.out, (pos >> 6) + (uint32_t)P);
            if (partial) ob += WIN;
            if (tr >= A.nsteps) A.done = true;                                   // out of soft values (nsteps is a whole number of groups: met exactly)
            if (tr >= B.nsteps) B.done = true;
            next_thr = next_event();
        }
    }

    // chunk C of the period: tr % 120 == 20 C on entry
    template <int C> __device__ __forceinline__ void chunk(uint32_t& raw, uint32_t& c)
    {
        const Chunk K = unpack(raw);
        raw = fetch(c + 2); c++;
        if (tr + CS <= nsteps && next_thr > tr + CS) {                          // no look at the schedule due inside: straight-line code
            group<CS * C>(K); group<CS * C + 5>(K); group<CS * C + 10>(K); group<CS * C + 15>(K);
            tr += CS;
        } else {
            if (going()) { group<CS * C>(K); tr += GS; check<(CS * C + 4) % 24>(); }
            if (going()) { group<CS * C + 5>(K); tr += GS; check<(CS * C + 9) % 24>(); }
            if (going()) { group<CS * C + 10>(K); tr += GS; check<(CS * C + 14) % 24>(); }
            if (going()) { group<CS * C + 15>(K); tr += GS; check<(CS * C + 19) % 24>(); }
        }
    }

    // From the first soft value to the end of both sides.  Chunk c + 2 is requested before chunk c is stepped through.
    __device__ __forceinline__ void run()
    {
        next_thr = next_event();
        uint32_t c = 0, r0 = fetch(0), r1 = fetch(1);
        while (going()) {
            chunk<0>(r0, c); if (!going()) break;
            chunk<1>(r1, c); if (!going()) break;
            chunk<2>(r0, c); if (!going()) break;
            chunk<3>(r1, c); if (!going()) break;
            chunk<4>(r0, c); if (!going()) break;
            chunk<5>(r1, c);
        }
    }
};

}  // namespace sora
