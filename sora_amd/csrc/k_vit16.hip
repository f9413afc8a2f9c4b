// k_vit16.hip -- the K=7 trellis with SIXTEEN LANES PER FRAME PAIR: eight frames per wave (gfx950).
//
//   k_viterbi16 / k_viterbi16_11n   T11aViterbi<5000*8,48,256,24> / <..,312,192,36>: the same arithmetic, window schedule and
//                                   trace-back as k_viterbi (k_rx.hip, dev_viterbi.h), bit for bit, in a layout that needs
//                                   half the vector instructions per frame.  tools/emu_trellis16.py is the lane-level model
//                                   this file was written against (tests/test_trellis16_model.py runs it against the oracle).
//
// Why.  k_viterbi (64 lanes = the 64 states of one frame pair) spends, per frame pair and step, two operand instructions, an
// add, a cross-lane add and a packed minimum -- and every third step a v_permlane swap with its copy and wait states, because
// two of the six butterfly distances (32, 16) leave the 16-lane row a DPP move can reach.  It is bound by vector issue
// (profiles/r03_b_sq_counters_k_viterbi_pairstream.json: 200 M vector instructions, a wave executing one 62 % of its life).
//
// Layout.  The 64 states of a frame pair live in 16 lanes x 4 registers; a wave holds four pairs (one per row).  W = {0, 21,
// 42, 63} is a subgroup of (Z_2)^6 that the in-place butterfly (state -> rol6(state)) maps onto itself and whose members are
// orthogonal to every rotation of both generator polynomials (0155, 0117): the states s ^ w, w in W, have IDENTICAL branch
// metrics at every step.  A lane holds such a coset, register i <-> w_i.  The butterfly partner of s at step t is s ^ e_j,
// j = 5 - t mod 6, and with lane = c0 ^ c2 << 1 ^ c1 << 3 ^ (c3 ? 7 : 0) for the coset of c0 e0 + c1 e1 + c2 e2 + c3 e3:
//     e0, e2, e4 = e0 ^ e2 ^ 21   ->  lane ^ 1, lane ^ 2, lane ^ 3 (and register ^ 1)     quad_perm
//     e1, e3, e5 = e1 ^ e3 ^ 42   ->  lane ^ 8, lane ^ 7, lane ^ 15 (and register ^ 2)    row_ror:8, row_half_mirror, row_mirror
// Every exchange is ONE row-local DPP move folded into its add (v_add_u32_dpp) plus a register renaming: no v_permlane swaps,
// no wait states, and the step's two operands (P and K - P + mark, dev_viterbi.h) serve all four registers -- which of the two
// a register adds to its own metric is a compile-time property of (step, register) XOR a per-lane bit that is folded into the
// lane's masks exactly as in k_viterbi.  Per step and wave: 2 operand instructions + 4 x (add, add_dpp, pk_min) for EIGHT
// frames (k_viterbi: 5 to 8 for two).
//
// Operands.  The four rows decode different pairs, so the operands are per-lane values.  Lane (row, 2 j + f) fetches soft
// values j, j + 8 (, j + 16) of the chunk from frame f's stream (rx_types.h: a byte that is the high byte of the 16-bit metric
// field; byte loads, two chunks ahead -- vector loads return in order, so the look-ahead is just a deeper vmcnt) and writes
// them into the high bytes of its slots of the row's operand table in LDS (the other formats: a 16-bit load, a shift, a mask); four to six broadcast ds_read_b128 then hand every lane the
// chunk's operands (field A | field B << 16).  Round 3 first read ready-made operand dwords from HBM (264 MB per call
// written and read; now 50).
//
// Trace-back.  The survivor ring is indexed by rev6(state) as in k_viterbi (the next index is the low six bits of the byte
// read), one 128-byte table per row and block.  The walk is lane-parallel instead of readlane-serial: every lane walks the
// path of frame (row, lane & 1) with one LDS read per block, the eight paths of the wave side by side, and keeps the path's
// bytes in registers: a whole window leaves as dwords from the lane that owns the frame, anything else through the rows'
// lanes byte by byte (trace16, dev_vit16.h).  Per window ~450 instructions for eight frames (k_viterbi: ~400 for two).
//
// Cost.  Eight frames per wave means 512 waves for the 4096-frame batch of BASELINE configs[2]: alone on the chip this kernel
// is slower than k_viterbi (half the SIMDs idle), with several calls in flight it is faster; sora_rx_set_trellis selects.
#include <hip/hip_runtime.h>

#include "dev_vit16.h"

namespace sora {

namespace {

// The whole-frame form: one serial chain per frame, the window schedule of the frame itself, and a fast loop with a two-table operand hand-over.
template <int CR, int WIN, int LOOK, int BITS>
__device__ __forceinline__ void forward16(Lds16<WIN, LOOK>& S, const uint8_t* __restrict__ soft, uint32_t my_soft_off, uint32_t my_nsoft,
                                          uint32_t nstepsA, uint32_t nstepsB, uint32_t my_tr_end, bool my_valid, uint8_t* my_out)
{
    using F16 = Forward16<CR, WIN, LOOK, BITS>;
    using Chunk = typename F16::Chunk;
    using Raw = typename F16::Raw;
    constexpr int GS = F16::GS;
    F16 F;
    F.init(S, soft, my_soft_off, 0, max(my_nsoft, 1u) - 1u, 0x18u * kFld, wave_max_u32(max(nstepsA, nstepsB)));   // ALL_INIT0 / ALL_INIT (viterbilut.h:22-30)

    uint32_t ob = 0;
    bool my_done = !my_valid;

    auto trace = [&](uint32_t my_cnt, int t24_last) {
        trace16<WIN, LOOK>((unsigned)(uintptr_t)&S, F.V.U[0], F.V.U[1], F.V.U[2], F.V.U[3], F.tr, ob, F16::pos_of(F.pos, t24_last / 8), (uint32_t)(t24_last % 8), my_cnt, my_out);
    };
    auto next_event = [&]() -> uint32_t {
        const uint32_t mine = my_done ? kNever : my_tr_end;
        return min(ob + (uint32_t)(WIN + LOOK + 6), wave_min_u32(mine));
    };
    F.next_thr = next_event();
    F.all_done = wave_min_u32(my_done ? 1u : 0u) != 0u;
    auto check = [&](int t24_last) {                                            // trace-back schedule (viterbi.hpp:196-214), per frame
        if (F.tr >= F.next_thr) {
            const bool partial = F.tr >= ob + (uint32_t)(WIN + LOOK + 6);
            uint32_t cnt = 0;
            if (!my_done) {
                if (F.tr >= my_tr_end) { cnt = my_tr_end - ob - 6; my_done = true; }
                else if (partial) cnt = WIN;
            }
            if (wave_max_u32(cnt) != 0u) { trace(cnt, t24_last); F.clear_ops(S); }
            if (partial) ob += WIN;
            F.next_thr = next_event();
            F.all_done = wave_min_u32(my_done ? 1u : 0u) != 0u;
        }
    };

    // The fast loop's operand hand-over, off the critical path (round 4).  unpack() writes a chunk's fields, reads the row's table back and uses the
    // operands at once: one LDS round trip per 12 steps sits in a lone wave's dependence chain (SQ_WAIT_ANY 21 % of its cycles,
    // profiles/r04_a_sq_counters_alone.json).  Here chunk c + 1's fields are written at the START of chunk c into the other of two tables and read
    // back in the MIDDLE of chunk c: by the time chunk c + 1 begins its operands have long been in registers.
    uint16_t* my_ops2[2] = { &S.ops2[0][F.row][F.my_j][F.half], &S.ops2[1][F.row][F.my_j][F.half] };
    const uint4* row_ops2[2] = { reinterpret_cast<const uint4*>(&S.ops2[0][F.row][0][0]), reinterpret_cast<const uint4*>(&S.ops2[1][F.row][0][0]) };
    auto stage = [&](const Raw& R, int t) { F.put(R, my_ops2[t]); };
    auto collect = [&](int t) -> Chunk { lds_fence(); return F16::get(row_ops2[t]); };
    auto fast_chunk_mid = [&](const Chunk& K, int h, Chunk& Knext, int tnext) {
#pragma unroll
        for (int g = 0; g < 12 / GS; g++) {
            if (g == (12 / GS) / 2) Knext = collect(tnext);
            F.group(K, h, g * GS);
        }
        F.tr += 12;
    };

    // Vector loads return in order: chunk c + 2 is requested before chunk c is stepped through.  Four fetch buffers in fixed roles, two rows
    // per turn of the fast loop, so that no buffer is ever copied.
    uint32_t c = 0;
    Raw b0 = F.fetch(0), b1 = F.fetch(1), b2, b3;
    while (F.going()) {
        const uint32_t lim = min(F.nsteps, F.next_thr - 1);
        uint32_t rows = lim > F.tr ? (lim - F.tr) / 24 : 0;                     // rows that certainly need no look at the schedule
        if (rows >= 2) {
            // invariant at the top of a turn: Ka = chunk c's operands (in registers), b1 / b2 = the raw values of chunks c + 1 / c + 2 (requested)
            Chunk Ka, Kb;
            b2 = F.fetch(c + 2);
            stage(b0, 0); Ka = collect(0); lds_fence();
            if constexpr (BITS == kSoftScaled) {
                // the handle's padded buffer: no clamp, one address register per turn and the turn's four chunks at compile-time offsets from it
                uint32_t p = F.fast_base(c);
                for (; rows >= 2; rows -= 2) {
                    b3 = F.template fetch_at<3>(p); stage(b1, 1); fast_chunk_mid(Ka, 0, Kb, 1);
                    b0 = F.template fetch_at<4>(p); stage(b2, 0); fast_chunk_mid(Kb, 1, Ka, 0);
                    F.end_row();
                    b1 = F.template fetch_at<5>(p); stage(b3, 1); fast_chunk_mid(Ka, 0, Kb, 1);
                    b2 = F.template fetch_at<6>(p); stage(b0, 0); fast_chunk_mid(Kb, 1, Ka, 0);
                    F.end_row();
                    c += 4; p += 4u * (uint32_t)F16::CW;
                }
            } else {
                for (; rows >= 2; rows -= 2) {
                    b3 = F.fetch(c + 3); stage(b1, 1); fast_chunk_mid(Ka, 0, Kb, 1);
                    b0 = F.fetch(c + 4); stage(b2, 0); fast_chunk_mid(Kb, 1, Ka, 0);
                    F.end_row();
                    b1 = F.fetch(c + 5); stage(b3, 1); fast_chunk_mid(Ka, 0, Kb, 1);
                    b2 = F.fetch(c + 6); stage(b0, 0); fast_chunk_mid(Kb, 1, Ka, 0);
                    F.end_row();
                    c += 4;
                }
            }
            // (the tables share their bytes with unpack()'s and the trace-back's: nothing of them is pending past here)
            lds_fence();
            // b0 holds chunk c's raw values, b1 / b2 those of c + 1 / c + 2: what the code below expects of b0, b1
        }
        if (!(F.tr < F.nsteps)) break;
        b2 = F.fetch(c + 2);
        if (rows) F.fast_chunk(F.unpack(b0), 0); else F.chunk(F.unpack(b0), 0, check);
        if (!F.going()) break;
        b3 = F.fetch(c + 3);
        if (rows) F.fast_chunk(F.unpack(b1), 1); else F.chunk(F.unpack(b1), 1, check);
        F.end_row();
        b0 = b2; b1 = b3;
        c += 2;
    }
}

// One wave per workgroup: wave w of code-rate list r decodes pairs 4w .. 4w+3 of the list (jobs 8w .. 8w+7), one pair per 16-lane row.
template <int WIN, int LOOK, int BITS>
__device__ __forceinline__ void viterbi16_body(const VitJob* __restrict__ jobs, const uint32_t* __restrict__ njobs3, uint32_t njobs_single, uint32_t stride,
                                               const uint8_t* __restrict__ soft, uint8_t* __restrict__ out)
{
    __shared__ Lds16<WIN, LOOK> S;
    uint32_t n[3] = { njobs_single, 0, 0 };
    if (njobs3) { n[0] = njobs3[0]; n[1] = njobs3[1]; n[2] = njobs3[2]; }
    uint32_t w = uni(blockIdx.x), list = 0;
    while (list < 3 && w >= (n[list] + 7) / 8) { w -= (n[list] + 7) / 8; list++; }
    if (list >= 3) return;
    const uint32_t njobs = uni(n[list]);
    jobs += (size_t)list * stride;
    const unsigned lane = threadIdx.x & 63, row = lane >> 4, half = lane & 1u;
    const uint32_t fa = 8u * w + 2u * row, fb = fa + 1u;
    const bool hasA = fa < njobs, hasB = fb < njobs;
    const VitJob& GA = jobs[hasA ? fa : 8u * w];                                // an empty row reads the wave's first pair (its operands are never used)
    const VitJob& GBj = jobs[hasB ? fb : (hasA ? fa : 8u * w)];
    const uint32_t code_rate = uni(jobs[8u * w].code_rate);
    const uint32_t gsd = code_rate == 0 ? 2u : code_rate == 2 ? 4u : 3u, gss = code_rate == 0 ? 1u : code_rate == 2 ? 3u : 2u;
    const uint32_t nstepsA = hasA ? GA.nsoft / gsd * gss : 0u, nstepsB = hasB ? GBj.nsoft / gsd * gss : 0u;
    const VitJob& Mine = half ? GBj : GA;
    const bool my_valid = half ? hasB : hasA;
    const uint32_t my_tr_end = Mine.length * 8u + 16u + 6u;
    uint8_t* my_out = out + Mine.out_off;
    if (code_rate == 0)      forward16<0, WIN, LOOK, BITS>(S, soft, Mine.soft_off, Mine.nsoft, nstepsA, nstepsB, my_tr_end, my_valid, my_out);
    else if (code_rate == 1) forward16<1, WIN, LOOK, BITS>(S, soft, Mine.soft_off, Mine.nsoft, nstepsA, nstepsB, my_tr_end, my_valid, my_out);
    else                     forward16<2, WIN, LOOK, BITS>(S, soft, Mine.soft_off, Mine.nsoft, nstepsA, nstepsB, my_tr_end, my_valid, my_out);
}

}  // namespace

__global__ void __launch_bounds__(64) k_viterbi16(const VitJob* __restrict__ jobs, const uint32_t* __restrict__ njobs3, uint32_t njobs_single, uint32_t stride,
        const uint8_t* __restrict__ soft, uint8_t* __restrict__ out)
{ viterbi16_body<256, 24, kSoftScaled>(jobs, njobs3, njobs_single, stride, soft, out); }
// the same decoder over three-bit streams in a caller's workspace (sora_hip_viterbi11a*: every fetch clamped, nothing assumed behind the streams)
__global__ void __launch_bounds__(64) k_viterbi16_p3(const VitJob* __restrict__ jobs, const uint32_t* __restrict__ njobs3, uint32_t njobs_single, uint32_t stride,
        const uint8_t* __restrict__ soft, uint8_t* __restrict__ out)
{ viterbi16_body<256, 24, 3>(jobs, njobs3, njobs_single, stride, soft, out); }
__global__ void __launch_bounds__(64) k_viterbi16_11n(const VitJob* __restrict__ jobs, const uint32_t* __restrict__ njobs3, uint32_t njobs_single,
        uint32_t stride, const uint8_t* __restrict__ soft, uint8_t* __restrict__ out)
{ viterbi16_body<192, 36, 8>(jobs, njobs3, njobs_single, stride, soft, out); }

}  // namespace sora
