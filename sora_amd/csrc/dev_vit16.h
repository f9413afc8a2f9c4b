// dev_vit16.h -- the pieces of the 16-lanes-per-frame-pair trellis layout shared by k_viterbi16 (k_vit16.hip: one serial chain per frame) and
// k_viterbi16w (k_vitwin.hip: the window-parallel form, round 5): the LDS layout, the coset <-> lane maps, the add-compare-select step, the
// lane's state and chunk machinery of the forward pass (Forward16: forward16 of k_vit16.hip and forward16w of dev_vitwin.h put their loops and
// schedules on top of it) and the lane-parallel trace-back of one window.  The layout itself is described at the top of k_vit16.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "dev_viterbi.h"

namespace sora {
namespace {

template <int WIN, int LOOK> struct Geom16 {
    static constexpr int kMaxWalk = (WIN + LOOK + 7) / 8 + 2;                   // 37 / 31 blocks a window's walk can touch
    static constexpr int P = kMaxWalk;                                          // ring period: the walk runs while nothing is being banked
    static constexpr int kPathBytes = 40;                                       // per frame: walk positions 0 .. kMaxWalk - 1
};

template <int WIN, int LOOK> struct Lds16 {
    // [block % P][row][rev6(state)] {frame A's byte, frame B's byte}: 18944 / 15872 B
    uint16_t ring[Geom16<WIN, LOOK>::P][4][64];
    union {
        uint32_t udump[4][64];                                                  // the metrics registers at a trace-back (the start state's unfinished block)
        // [row][operand of the chunk][frame]: the soft values as metric fields -- live only inside
        uint16_t ops[4][24][2];
        //   Forward16::unpack() / forward16's two alternating tables of its fast loop, never across a trace-back:
        uint16_t ops2[2][4][24][2];
    };                                                                          //   they share their bytes with the trace-back's register dump
    uint32_t path[8][Geom16<WIN, LOOK>::kPathBytes / 4];                         // [row * 2 + frame]: the bytes along the traced path in stream order (trace16's byte path only)
};                                                                              // 20288 / 17216 bytes: eight one-wave workgroups per CU (20480 each)

constexpr unsigned kW[4] = { 0u, 21u, 42u, 63u };

__device__ __forceinline__ unsigned v_of_lane(unsigned l)                       // coset representative (bits e0..e3) held by lane l of a row
{
    const unsigned b0 = l & 1u, b1 = (l >> 1) & 1u, b2 = (l >> 2) & 1u, b3 = (l >> 3) & 1u;
    const unsigned c3 = b2, c1 = b3, c0 = b0 ^ c3, c2 = b1 ^ c3;
    return c0 | (c1 << 1) | (c2 << 2) | (c3 << 3);
}
__device__ __forceinline__ unsigned lane_of_v(unsigned v)                       // inverse: lane of the coset with representative v (4 bits)
{
    const unsigned c0 = v & 1u, c1 = (v >> 1) & 1u, c2 = (v >> 2) & 1u, c3 = (v >> 3) & 1u;
    return c0 ^ (c2 << 1) ^ (c1 << 3) ^ (c3 ? 7u : 0u);
}
__device__ __forceinline__ unsigned rev6u(unsigned x) { return __brev(x) >> 26; }

template <int CTRL> __device__ __forceinline__ unsigned dppx(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true); }

// the partner's metric for phase ph = t mod 6: lane ^ {15, 3, 7, 2, 8, 1}
__device__ __forceinline__ unsigned partner(unsigned v, int ph)
{
    switch (ph) {
    case 0: return dppx<0x140>(v);                                              // row_mirror:      lane ^ 15   (e5; register ^ 2)
    case 1: return dppx<0x1B>(v);                                               // quad_perm [3,2,1,0]: ^ 3     (e4; register ^ 1)
    case 2: return dppx<0x141>(v);                                              // row_half_mirror: lane ^ 7    (e3)
    case 3: return dppx<0x4E>(v);                                               // quad_perm [2,3,0,1]: ^ 2     (e2)
    case 4: return dppx<0x128>(v);                                              // row_ror:8:       lane ^ 8    (e1)
    default: return dppx<0xB1>(v);                                              // quad_perm [1,0,3,2]: ^ 1     (e0)
    }
}

struct Vit16 {
    unsigned U[4];           // register i: the metrics of state (coset of the lane) ^ kW[i]; (field B << 16) | field A as in dev_viterbi.h
    unsigned MX[24];         // mask of the mark-carrying operand per t mod 24 (for lanes whose coset bit j is set: complemented, with the mark)
    unsigned MY[6];          // mask of the second operand of a two-input step per t mod 6
    unsigned sadr[3][4];     // LDS byte address (without the block's position) of the ring entry of register i at the end of block jb of a row
};

// WHICH 0: (A,B) two soft values, 1: A only, 2: B only.  t24 = step index mod 24 (a constant after unrolling).  pos512 = the ring
// position of the row's first block, in bytes (wave-uniform).
template <int WHICH, int P>
__device__ __forceinline__ void acs16(Vit16& V, int t24, unsigned a, unsigned b, unsigned pos512[3])
{
    const int ph = t24 % 6, k = t24 % 8;
    const unsigned Kp = (WHICH == 0 ? 14u : 7u) * kFld + (kOne << k);           // K + mark
    unsigned bm;
    if (WHICH == 0)      bm = (a ^ V.MX[t24]) + (b ^ V.MY[ph]);
    else if (WHICH == 1) bm = a ^ V.MX[t24];
    else                 bm = b ^ V.MX[t24];
    const unsigned bo = Kp - bm;
    const int rx = ph == 0 ? 2 : ph == 1 ? 1 : 0;
    unsigned N[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned X = V.U[i], Y = partner(V.U[i ^ rx], ph);
        const bool wb = (kW[i] >> (5 - ph)) & 1u;                               // the register's half of the role bit (the lane's half is in the masks)
        N[i] = wb ? pk_min16(X + bo, Y + bm) : pk_min16(X + bm, Y + bo);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) V.U[i] = N[i];
    if (k == 7) {                                                               // end of an 8-step block: bank the path histories, clear the marks
        const int jb = t24 / 8;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned w = bank_word(V.U[i]);
            const unsigned addr = V.sadr[jb][i] + pos512[jb];
            asm volatile("ds_write_b16 %0, %1" : : "v"(addr), "v"(w) : "memory");
            V.U[i] &= 0xFE00FE00u;
        }
    }
}

__device__ __forceinline__ unsigned row_min_u32(unsigned v)                     // minimum over the 16 lanes of the row, in every lane
{
    v = min(v, dppx<0xB1>(v)); v = min(v, dppx<0x4E>(v)); v = min(v, dppx<0x141>(v)); v = min(v, dppx<0x128>(v));
    return v;
}
__device__ __forceinline__ unsigned row_pkmin(unsigned v)
{
    v = pk_min16(v, dppx<0xB1>(v)); v = pk_min16(v, dppx<0x4E>(v)); v = pk_min16(v, dppx<0x141>(v)); v = pk_min16(v, dppx<0x128>(v));
    return v;
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)dpp_min_u32_wave(v)); }
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) { return ~wave_min_u32(~v); }

// The forward pass of a wave in this layout, less its loop and its schedule: the lane's metrics and masks, its part in fetching a chunk of soft values and handing
// them round the row, the steps of a chunk, the ring position.  The form on top owns what ends a run of steps (next_thr, all_done, its check()).
template <int CR, int WIN, int LOOK, int BITS>
struct Forward16 {
    static constexpr int P = Geom16<WIN, LOOK>::P, GB = Puncture<CR>::GB, GS = Puncture<CR>::GS, CW = Puncture<CR>::CW;
    static constexpr int NV = Puncture<CR>::NV;                                 // soft values a lane fetches per chunk: operands j, j + 8 (, j + 16) of its frame
    struct Chunk { uint32_t v[CW]; };
    struct Raw { SoftRaw r[NV]; };

    Vit16 V;
    unsigned row, half;                                                         // this lane's frame: (row, half)
    uint32_t my_j;
    SoftCursor<BITS, CW> cur[NV];
    uint32_t my_base;                                                           // byte offset (from the soft base) of operand j of chunk 0, unclamped (fetch_at)
    const uint8_t* soft;
    uint16_t* my_ops;
    const uint4* row_ops;
    uint32_t pos;                                                               // ring position of the current row's first block, in BYTES: 512 (block index % P)
    unsigned pos512[3];
    uint32_t tr, nsteps;                                                        // steps taken / of the wave's longest side (wave-uniform)
    uint32_t next_thr;
    bool all_done;

    // start: the metric of every state but state 0 (both halves); my_soft_off, my_first, my_last: this lane's frame's stream, the value of its first step, its last
    // value (fetches past it repeat it: well-formed operands nobody uses)
    __device__ __forceinline__ void init(Lds16<WIN, LOOK>& S, const uint8_t* __restrict__ soft_, uint32_t my_soft_off, uint32_t my_first, uint32_t my_last, unsigned start,
                                         uint32_t nsteps_)
    {
        const unsigned lane = threadIdx.x & 63, l16 = lane & 15;
        row = lane >> 4; half = lane & 1u;
        const unsigned v0 = v_of_lane(l16);
        nsteps = nsteps_;
#pragma unroll
        for (int i = 0; i < 4; i++) V.U[i] = (v0 ^ kW[i]) == 0 ? 0u : start;
        const unsigned ring_base = (unsigned)(uintptr_t)&S.ring[0][0][0];       // (the low half of a flat LDS address is the LDS offset)
#pragma unroll
        for (int jb = 0; jb < 3; jb++)
#pragma unroll
            // (8 jb + 8) mod 6
            for (int i = 0; i < 4; i++) V.sadr[jb][i] = ring_base + ((row * 64u + rev6u(rol6(v0 ^ kW[i], jb == 0 ? 2 : jb == 1 ? 4 : 0))) << 1);
#pragma unroll
        for (int t = 0; t < 24; t++) {
            const int ph = t % 6, k = t % 8;
            const unsigned n = rol6(v0, ph + 1);                                // register 0's state after the step (all four registers agree on the masks)
            const bool vb = (v0 >> (5 - ph)) & 1u;                              // the lane's half of the role bit
            const unsigned ma = (__popc(n & 0155) & 1) ? 7u * kFld : 0u, mb = (__popc(n & 0117) & 1) ? 7u * kFld : 0u;
            const unsigned mx = Puncture<CR>::which_of(ph) == 2 ? mb : ma;
            V.MX[t] = vb ? ((mx ^ (7u * kFld)) | (kOne << k)) : mx;
            if (t < 6) V.MY[t] = vb ? (mb ^ (7u * kFld)) : mb;
        }
        tr = 0; pos = 0;
        my_j = l16 >> 1;
#pragma unroll
        for (int v = 0; v < NV; v++) cur[v].init(my_soft_off, my_first + my_j + 8u * v, my_last);
        my_base = my_soft_off + my_first + my_j;
        soft = soft_;
        my_ops = &S.ops[row][my_j][half];
        row_ops = reinterpret_cast<const uint4*>(&S.ops[row][0][0]);
        set_row_pos();
        clear_ops(S);
    }
    __device__ __forceinline__ bool going() const { return tr < nsteps && !all_done; }

    __device__ __forceinline__ void normalize()                                 // Normalize (viterbicore.h:444-465): the row's minimum, both frames
    {
        const unsigned m = row_pkmin(pk_min16(pk_min16(V.U[0], V.U[1]), pk_min16(V.U[2], V.U[3])));
#pragma unroll
        for (int i = 0; i < 4; i++) V.U[i] -= m;
    }
    // The position jb blocks on.  It is kept in bytes and wrapped by one unsigned minimum (p < 512 P: p - 512 P is huge unless p has passed the ring's end), so a
    // banked block costs the scalar unit an add, a subtract and a minimum -- as a block index it was add, shift, add, compare, select.
    static __device__ __forceinline__ uint32_t pos_of(uint32_t p, int jb) { const uint32_t q = p + 512u * (uint32_t)jb; return min(q, q - 512u * (uint32_t)P); }
    __device__ __forceinline__ void set_row_pos()
    {
        pos512[0] = pos; pos512[1] = pos_of(pos, 1); pos512[2] = pos_of(pos512[1], 1);
    }
    __device__ __forceinline__ void end_row() { pos = pos_of(pos512[2], 1); set_row_pos(); }
    __device__ __forceinline__ Raw fetch(uint32_t c) const                      // chunk c: the loads only
    {
        Raw R;
#pragma unroll
        for (int v = 0; v < NV; v++) R.r[v] = cur[v].fetch(soft, c);
        return R;
    }
    // a chunk's fields into the lane's slots of an operand table (operand j + 8 v; slots up to 23 exist, those past CW are never read) ...
    __device__ __forceinline__ void put(const Raw& R, uint16_t* mine) const
    {
#pragma unroll
        for (int v = 0; v < NV; v++) soft_put(mine + 16 * v, cur[v], R.r[v]);
    }
    // The receive handle's bytes (kSoftScaled) fill only the high byte of a slot: the low bytes of both tables are zeroed when the wave starts and again behind every
    // trace-back, whose register dump (Lds16::udump) lies over them -- three stores per lane and 256 steps.
    __device__ __forceinline__ void clear_ops(Lds16<WIN, LOOK>& S) const
    {
        if constexpr (BITS == kSoftScaled) {
            static_assert(sizeof(S.ops2) == 3 * 64 * 4, "three dwords per lane");
            uint32_t* z = reinterpret_cast<uint32_t*>(&S.ops2[0][0][0][0]) + (threadIdx.x & 63);
            z[0] = 0u; z[64] = 0u; z[128] = 0u;
            lds_fence();
        }
    }
    // The same chunk's loads without the clamp, for a loop that knows the buffer behind the streams to be padded (rx_types.h: kSoftPad): the address is p + a
    // compile-time offset, p = fast_base(c0) the lane's byte offset of operand j of chunk c0 -- one register, advanced once per turn of the loop by whoever calls.
    __device__ __forceinline__ uint32_t fast_base(uint32_t c0) const { return my_base + c0 * (uint32_t)CW; }
    template <int DC> __device__ __forceinline__ Raw fetch_at(uint32_t p) const
    {
        static_assert(BITS == kSoftScaled, "one byte per value");
        Raw R;
#pragma unroll
        for (int v = 0; v < NV; v++) { R.r[v].sh = 0; R.r[v].w = soft[(size_t)p + (size_t)(DC * CW + 8 * v)]; }
        return R;
    }
    // ... and the row's table into every lane's registers
    static __device__ __forceinline__ Chunk get(const uint4* table)
    {
        Chunk K;
#pragma unroll
        for (int i = 0; i < (CW + 3) / 4; i++) {
            const uint4 x = table[i];
            K.v[4 * i] = x.x; K.v[4 * i + 1] = x.y;
            if (4 * i + 2 < CW) { K.v[4 * i + 2] = x.z; K.v[4 * i + 3] = x.w; }
        }
        return K;
    }
    __device__ __forceinline__ Chunk unpack(const Raw& R) const                 // ... their values -> the row's operand table -> every lane's registers
    {
        put(R, my_ops);
        lds_fence();
        const Chunk K = get(row_ops);
        lds_fence();
        return K;
    }
    // one puncture group = GS steps; i0 = step inside the chunk, h = half of the 24-step row
    __device__ __forceinline__ void group(const Chunk& K, int h, int i0)
    {
        const int k0 = i0 / GS * GB, t24 = 12 * h + i0;
        acs16<0, P>(V, t24, K.v[k0], K.v[k0 + 1], pos512);                      // ACS(A,B)
        if (CR != 0) acs16<1, P>(V, t24 + 1, K.v[k0 + 2], 0, pos512);           // ACS(A)     2/3, 3/4 (viterbi.hpp:173-187)
        if (CR == 2) acs16<2, P>(V, t24 + 2, 0, K.v[k0 + 3], pos512);           // ACS(B)     3/4
        if ((t24 + GS) % 8 == 0) normalize();                                   // (trellis index & 7) == 0 after a group
    }
    __device__ __forceinline__ void fast_chunk(const Chunk& K, int h)           // 12 steps, no trace-back due inside: straight-line code
    {
#pragma unroll
        for (int g = 0; g < 12 / GS; g++) group(K, h, g * GS);
        tr += 12;
    }
    // up to 12 steps with the schedule examined after every group (check(t24 of the group's last step): the form's)
    template <typename CHECK> __device__ __forceinline__ void slow_chunk(const Chunk& K, int h, CHECK& check)
    {
#pragma unroll
        for (int g = 0; g < 12 / GS; g++) {
            if (going()) {
                group(K, h, g * GS);
                tr += GS;
                check(12 * h + g * GS + GS - 1);
            }
        }
    }
    template <typename CHECK> __device__ __forceinline__ void chunk(const Chunk& K, int h, CHECK& check)   // tr % 24 == 12 h on entry
    {
        if (tr + 12 <= nsteps && next_thr > tr + 12) fast_chunk(K, h); else slow_chunk(K, h, check);
    }
};

// Trace-back of one window for every frame of the wave whose count is non-zero (my_cnt: this lane's frame = (row, lane & 1)); kept out of
// line (it is reached from every puncture group of the slow path), so everything arrives by value and the LDS block by its offset.
// pj = ring position, in bytes (Forward16::pos), of block j = (tr - 1) >> 3; k = index in its 8-step block of the last step taken.
// LANE_OB (k_vitwin.hip): ob_ is a per-lane value -- the units a wave decodes hand out their bits at different positions of their frames.
//
// The bytes along the traced path stay in registers.  The walk is unrolled in full, so walk position i is a compile-time place: the bytes are packed four to a
// register in the order the decoded stream wants them (stream byte s = walk position kMaxWalk - 1 - s; two raw ring words -> one register -> v_perm_b32 picks
// this frame's byte of each pair), and decoded byte z of the window is bits 8 (s0 + z) + 6 .. + 13 of that stream, s0 = kMaxWalk - 1 - (j - ob / 8).
//   * a whole window (count WIN) of the whole-frame form always has s0 = 1: a decoded dword is one v_alignbit_b32 by 14 of two neighbouring registers, and the
//     lane that owns the frame (lane & 15 < 2) stores the window's WIN / 8 bytes as dwords;
//   * any other case in the wave -- a frame's last, partial window, an output that is not dword-aligned, and every trace-back of the LANE_OB form, whose units put
//     s0 anywhere and their bytes at any alignment -- takes the byte path: the registers go to Lds16::path as dwords, and the row's lanes assemble and store the
//     bytes one by one as before.
template <int WIN, int LOOK, bool LANE_OB = false>
__device__ __noinline__ void trace16(unsigned lds_off, unsigned U0, unsigned U1, unsigned U2, unsigned U3, uint32_t tr_, uint32_t ob_, uint32_t pj_, uint32_t k_,
                                     uint32_t my_cnt, uint8_t* my_out)
{
    using G = Geom16<WIN, LOOK>;
    constexpr int P = G::P, K = G::kMaxWalk;
    constexpr int NR = K - 1, NF = NR / 4, NW = K / 4 + 1;                      // ring words read by the walk; registers they fill; registers of the stream (position 0 included)
    static_assert(NR % 4 == 0 || NR % 4 == 2, "the walk's words are packed in pairs");
    static_assert(NW * 4 <= G::kPathBytes && NW >= WIN / 32 + 1, "the stream's registers hold a window and fit Lds16::path");
    typedef __attribute__((address_space(3))) Lds16<WIN, LOOK> lds_t;
    typedef __attribute__((address_space(3))) const uint16_t lds_u16;
    lds_t& S = *(lds_t*)(uintptr_t)lds_off;
    auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    const uint32_t tr = uni(tr_), ob = LANE_OB ? ob_ : uni(ob_), pj = uni(pj_), k = uni(k_);
    const unsigned lane = threadIdx.x & 63, row = lane >> 4, l16 = lane & 15, half = lane & 1u;
    const unsigned v0 = v_of_lane(l16);
    const unsigned U[4] = { U0, U1, U2, U3 };
    const uint32_t j = (tr - 1) >> 3, nn = tr - 8u * j, m_lo = ob >> 3;
    const unsigned rowbase = (unsigned)(uintptr_t)&S.ring[0][row][0], sh = 8u * half;
    auto ring_j = [&](unsigned idx) -> unsigned { return *(lds_u16*)(uintptr_t)(rowbase + pj + (idx << 1)); };   // block j's entry of this row
    // the metrics registers -> LDS (the start state's unfinished block is read from there); the ring writes of this block are visible after the fence
#pragma unroll
    for (int i = 0; i < 4; i++) S.udump[i][lane] = U[i];
    lds_fence();
    // arg-min with the reference's tie-break metric << 8 | state << 2 (viterbicore.h:479-524), metric = 2u + last decision
    unsigned key[2] = { 0xFFFFFFFFu, 0xFFFFFFFFu };
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned st = rol6(v0 ^ kW[i], tr);
        unsigned lastA, lastB;
        if (k == 7) { const unsigned w = ring_j(rev6u(st)); lastA = (w >> 7) & 1u; lastB = (w >> 15) & 1u; }
        else { lastA = (U[i] >> k) & 1u; lastB = (U[i] >> (17 + k)) & 1u; }
        const unsigned mA = ((U[i] & 0xFFFFu) >> 9 << 1) | lastA, mB = (U[i] >> 25 << 1) | lastB;
        key[0] = min(key[0], (mA << 8) | (st << 2)); key[1] = min(key[1], (mB << 8) | (st << 2));
    }
    const unsigned kA = row_min_u32(key[0]), kB = row_min_u32(key[1]);
    const unsigned st = ((half ? kB : kA) >> 2) & 0x3Fu;                        // this lane's frame's start state
    // the slot holding st now: state0 = ror6(st, tr), register from bits 4 / 5, lane from the coset representative
    const unsigned s0 = rol6(st, 6u - tr % 6u);
    const unsigned b4 = (s0 >> 4) & 1u, b5 = (s0 >> 5) & 1u;
    const unsigned ri = b4 | (b5 << 1);
    const unsigned sl = lane_of_v((s0 ^ (b4 ? 21u : 0u) ^ (b5 ? 42u : 0u)) & 15u);
    const unsigned Ust = S.udump[ri][row * 16u + sl];
    unsigned H;
    if (nn == 8) H = (ring_j(rev6u(st)) >> sh) & 0xFFu;
    else H = ((Ust >> (17u * half)) & 0xFFu) & ((1u << nn) - 1u);
    unsigned q = rev6u(((st >> nn) | rev6u(H & 0x3Fu)) & 0x3Fu);                 // ring index at column 8j
    // The walk, unrolled in full: the ring position steps down by 512 (mod 512 P), a scalar -- its row's byte offset is one v_lshl_add off the dependence
    // chain -- so that a block costs the chain ds_read -> bfe -> lshl_add -> ds_read and half an instruction to pair its word with its neighbour's.
    unsigned pr[NR / 2];                                                        // pair n: the raw words of stream bytes 2n (low half) and 2n + 1
    uint32_t p = pj;
#pragma unroll
    for (int i = 1; i < K; i++) {                                               // always the full length: blocks below the window are read and never used
        uint32_t d;
        p = __builtin_sub_overflow(p, 512u, &d) ? 512u * (uint32_t)(P - 1) : d;     // (s_sub_u32, s_cselect_b32 on its borrow)
        unsigned base = rowbase + p;
        // (one register: the chain's add is then v_lshl_add, not a three-input add behind a shift)
        asm volatile("" : "+v"(base));
        const unsigned raw = *(lds_u16*)(uintptr_t)(base + (q << 1));
        q = __builtin_amdgcn_ubfe(raw, sh, 6u);
        const int s = K - 1 - i;
        if (s & 1) pr[s >> 1] = raw << 16; else pr[s >> 1] |= raw;
    }
    // this frame's byte of each word of two pairs -> four stream bytes; walk position 0 (H) ends the stream
    unsigned R[NW];
    const unsigned sel = 0x06040200u + 0x01010101u * half;
#pragma unroll
    for (int w = 0; w < NF; w++) R[w] = __builtin_amdgcn_perm(pr[2 * w + 1], pr[2 * w], sel);
    if (NR % 4 == 0) R[NF] = H;
    else R[NF] = __builtin_amdgcn_perm(H, pr[2 * NF], 0x0C040200u + 0x00000101u * half);
    // decoded byte m = (block m >> 6) | (block m + 1 & 0x3F) << 2; block m sits at walk position j - m
    const uint32_t sfirst = (uint32_t)(K - 1) - (j - m_lo);                     // stream byte of the window's first block
    bool fast = !LANE_OB;
    if (!LANE_OB) {
        const bool whole = my_cnt == (uint32_t)WIN && sfirst == 1u && (((uintptr_t)my_out + m_lo) & 3u) == 0;
        fast = __ballot(!(whole || my_cnt == 0)) == 0;
    }
    if (fast) {
        if (my_cnt != 0 && l16 < 2) {                                           // lane (row, half): its own frame's window, WIN / 8 bytes
            uint32_t* o = reinterpret_cast<uint32_t*>(my_out + m_lo);
#pragma unroll
            for (int dw = 0; dw < WIN / 32; dw++) o[dw] = __builtin_amdgcn_alignbit(R[dw + 1], R[dw], 14);
        }
    } else {
        __attribute__((address_space(3))) uint32_t* pw = S.path[row * 2u + half];
        if (l16 < 2) {
#pragma unroll
            for (int w = 0; w < NW; w++) pw[w] = R[w];
        }
        lds_fence();
        // Lane (l16 >> 1) of the row's eight lanes with this `half` takes bytes m_lo + (l16 >> 1) + 8 z.
        __attribute__((address_space(3))) const uint8_t* pth = (__attribute__((address_space(3))) const uint8_t*)pw;
        const uint32_t nbytes = my_cnt >> 3;
        for (uint32_t z = l16 >> 1; z < nbytes; z += 8) {
            const uint32_t sb = sfirst + z;                                     // <= kMaxWalk - 2: the window ends at least one block below the start column
            my_out[m_lo + z] = (uint8_t)(((unsigned)pth[sb] >> 6) | (((unsigned)pth[sb + 1] & 0x3Fu) << 2));
        }
    }
    lds_fence();
}

}  // namespace
}  // namespace sora
