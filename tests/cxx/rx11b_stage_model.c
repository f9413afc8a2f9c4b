/* TEST INFRASTRUCTURE -- the bricks of the 802.11b receive graph (CreateDemodGraph, kernel/bb/demod11/fb11bdemod_config.hpp:122-172) ONE BY ONE: array in,
 * array and state out.  What the stage entry points sora_hip_*11b (include/sora_hip.h, k_11b.hip) are compared with, stream by stream.
 *
 * tests/cxx/rx11b_ext_model.c states the same bricks inside its walk over a whole capture, each calling the next; this file RESTATES their bodies with the
 * calls to the next brick taken out and the state in the records of include/sora_hip.h (sora_*11b_state, all 32-bit words), so that a brick can be run alone.
 * tests/test_11b_stage_model_cpu.py composes them again (rx11b_stage_model.first_event) and pins the composition to that file and to the oracle.
 * Linked against nothing: the oracle library (so_init, so_g_crc_lut) is loaded first, with global symbols (tests/rx11b_stage_model.py). */
#include <string.h>
#include "so_internal.h"

enum { RATE_SYNC = 0, RATE_1M, RATE_2M, RATE_5P5M, RATE_11M };
enum { NO_PEAK_FOUND = 0, PEAK_FOUND, PEAK_VALID, PEAK_VALIDED, BARKER_SYNCED };
#define E_PLCP_HEADER_FAIL 0x80000005u
#define E_CRC32_FAIL       0x80000006u
#define E_FRAME_OK         0x00000001u
#define E_SFD_FAIL         0x80000004u
#define E_CS_TIMEOUT       0x80000007u
#define E_SFD_TIMEOUT      0x80000008u
#define E_SYNC_TIMEOUT     0x80000009u

/* the records of include/sora_hip.h */
typedef struct { so_c16 last_symbol; uint32_t byte_reg, is_even, reserved; } st_stream;
typedef struct { uint32_t average_energy, window[8], idx, count, power_detected, error_code, cca_pwr_threshold, update_cnt; so_c16 sum_dc, dc; } st_energy;
typedef struct { int32_t m_index, m_frag; } st_symt;
typedef struct { int32_t sync_flag, last_peak_cnt, m_max, search_count; so_c16 partial[10]; uint32_t error_code; } st_barker;
typedef struct { so_c16 last_symbol; uint32_t byte_reg, bit_one_found, bit_zero_found, word, bit_err_cnt, sync_cnt, rxrate_state, error_code; } st_sfd;
typedef struct { uint32_t error_code, data_rate_kbps, frame_length, rxrate_state; } st_plcp;
typedef struct { uint32_t error_code, frame_crc32; } st_sink;

/* ---- TDCRemove (dc.hpp:6-38): wrapping subtraction, bursts of 4 */
void st11b_dc_remove(const so_c16* in, uint32_t nbursts, so_c16 dc, so_c16* out)
{
    for (uint32_t i = 0; i < 4 * nbursts; i++) out[i] = so_c(so_w16(in[i].re - dc.re), so_w16(in[i].im - dc.im));
}

/* ---- TEnergyDetect::Process (cca.hpp:54-96) + TDCEstimator (dc.hpp:131-163): bursts until power is detected or an error is raised -> bursts consumed */
uint32_t st11b_energy_detect(const so_c16* in, uint32_t n, st_energy* s)
{
    uint32_t used = 0;
    while (used < n && !s->power_detected && s->error_code == 0) {
        const so_c16* v = in + 4 * used++;
        uint32_t ave = 0;
        for (int k = 0; k < 4; k++) ave = (uint32_t)so_w32((int64_t)(int32_t)ave + (so_sqnorm(v[k]) >> 5));
        s->average_energy = s->average_energy - s->window[s->idx] + ave;
        s->window[s->idx] = ave;
        if (++s->idx >= 8) s->idx = 0;
        s->count++;
        if (s->count >= 32) {
            if (s->count >= 100) { s->error_code = E_CS_TIMEOUT; continue; }
            if (s->average_energy >= s->cca_pwr_threshold) s->power_detected = 1;
        }
        if (!s->power_detected) {                                          /* energy gating: only low-power samples reach the DC estimator */
            so_c16 h = so_c(0, 0);
            for (int k = 0; k < 4; k++) h = so_c(so_w16(h.re + (v[k].re >> 5)), so_w16(h.im + (v[k].im >> 5)));
            s->sum_dc = so_c(so_w16(s->sum_dc.re + h.re), so_w16(s->sum_dc.im + h.im));
            if (s->update_cnt == 0) {
                s->dc = so_c(so_w16(s->dc.re + (s->sum_dc.re >> 2)), so_w16(s->dc.im + (s->sum_dc.im >> 2)));
                s->update_cnt = 8; s->sum_dc = so_c(0, 0);
            }
            s->update_cnt--;
        }
    }
    return used;
}

/* ---- TSymTiming::Process (symtiming.hpp:42-170) on nblocks blocks of 28 samples -> chips written (6, 7 or 8 per block); trace (or null): m_index behind each
 * block, before the next block's Decimation folds -1 and 4 back */
uint32_t st11b_symtiming(const so_c16* in, uint32_t nblocks, st_symt* s, so_c16* out, int32_t* trace)
{
    uint32_t nout = 0;
    for (uint32_t b = 0; b < nblocks; b++) {
        const so_c16* blk = in + 28 * (size_t)b;
        int idx = s->m_index;                                               /* Decimation (:66-83) */
        while (idx < 28) {
            if (idx < 0) { out[nout++] = blk[0]; s->m_index += 4; } else out[nout++] = blk[idx];
            idx += 4;
        }
        if (s->m_index >= 4) s->m_index = 0;
        int32_t sum[4] = { 0, 0, 0, 0 };                                    /* AdjustTiming (:118-170) */
        for (int i = 0; i < 28; i++) sum[i & 3] = so_w32((int64_t)sum[i & 3] + so_sqnorm(so_sra(blk[i], 3)));
        const int mi = s->m_index;
        const int early = (mi == 0) ? 3 : mi - 1, late = (mi == 3) ? 0 : mi + 1;
        if (sum[early] < sum[late]) {
            if (sum[mi] < sum[early]) { s->m_index++; s->m_frag = 0; }
            else if (sum[mi] < sum[late]) s->m_frag++;
        } else {
            if (sum[mi] < sum[late]) { s->m_index--; s->m_frag = 0; }
            else if (sum[mi] < sum[early]) s->m_frag--;
        }
        if (s->m_frag >= 4) { s->m_index++; s->m_frag = -3; }
        else if (s->m_frag <= -4) { s->m_index--; s->m_frag = 3; }
        if (trace) trace[b] = s->m_index;
    }
    return nout;
}

/* ---- TBarkerSync::Process (symtiming.hpp:229-313): chips swallowed until BARKER_SYNCED, or up to the chip that raises the time-out -> chips consumed */
uint32_t st11b_barker_sync(const so_c16* in, uint32_t n, st_barker* s)
{
    uint32_t used = 0;
    while (used < n && s->sync_flag != BARKER_SYNCED && s->error_code == 0) {
        const so_c16 x = in[used++];
        s->search_count++;
        if (s->search_count >= 11 * 4) { s->error_code = E_SYNC_TIMEOUT; break; }
        const so_c16 ss = so_sra(x, 4);                                     /* UpdateBarkerCorrelation (:296-313) */
        so_c16* p = s->partial;
#define SUB(a) so_c(so_w16((a).re - ss.re), so_w16((a).im - ss.im))
#define ADD(a) so_c(so_w16((a).re + ss.re), so_w16((a).im + ss.im))
        const so_c16 o = SUB(p[0]);
        p[0] = SUB(p[1]); p[1] = SUB(p[2]); p[2] = ADD(p[3]); p[3] = ADD(p[4]); p[4] = ADD(p[5]); p[5] = SUB(p[6]);
        p[6] = ADD(p[7]); p[7] = ADD(p[8]); p[8] = SUB(p[9]); p[9] = ss;
#undef SUB
#undef ADD
        const int corr = so_sqnorm(o);
        switch (s->sync_flag) {
        case NO_PEAK_FOUND:
            if (corr > s->m_max) { s->m_max = corr; s->last_peak_cnt = 1; }
            else if (++s->last_peak_cnt == 11) s->sync_flag = PEAK_FOUND;
            break;
        case PEAK_FOUND:
            s->m_max = corr / 2; s->last_peak_cnt = 1; s->sync_flag = PEAK_VALID;
            break;
        case PEAK_VALID:
            if (corr > s->m_max) { s->m_max = corr; s->last_peak_cnt = 0; s->sync_flag = NO_PEAK_FOUND; }
            else if (++s->last_peak_cnt == 11) s->sync_flag = PEAK_VALIDED;
            break;
        default:
            s->sync_flag = BARKER_SYNCED;                                   /* "just skip one more symbol" */
        }
    }
    return used;
}

/* ---- TBB11bDespread::QuickBarkerDespread (barkerspread.hpp:277-303): chips 1 and 4 are negated BEFORE the >> 4, chips 8-10 are subtracted after it; all in
 * wrapping int16 */
static so_c16 despread1(const so_c16 c[11])
{
    static const int pre_neg[8] = { 0, 1, 0, 0, 1, 0, 0, 0 };
    int16_t re[4] = { 0, 0, 0, 0 }, im[4] = { 0, 0, 0, 0 };
    for (int k = 0; k < 4; k++) {
        so_c16 v = c[k]; if (pre_neg[k]) v = so_c(so_neg16(v.re), so_neg16(v.im));
        re[k] = (int16_t)(v.re >> 4); im[k] = (int16_t)(v.im >> 4);
    }
    for (int k = 0; k < 4; k++) {
        so_c16 v = c[4 + k]; if (pre_neg[4 + k]) v = so_c(so_neg16(v.re), so_neg16(v.im));
        re[k] = so_w16(re[k] + (v.re >> 4)); im[k] = so_w16(im[k] + (v.im >> 4));
    }
    for (int k = 0; k < 3; k++) {
        re[k] = so_w16(re[k] - (c[8 + k].re >> 4)); im[k] = so_w16(im[k] - (c[8 + k].im >> 4));
    }
    return so_c(so_w16(re[0] + re[1] + re[2] + re[3]), so_w16(im[0] + im[1] + im[2] + im[3]));
}
void st11b_despread(const so_c16* in, uint32_t n, so_c16* out)
{
    for (uint32_t i = 0; i < n; i++) out[i] = despread1(in + 11 * (size_t)i);
}

static inline uint32_t dot_sign(so_c16 ref, so_c16 x)                      /* (ulong)(ref.re*s.re + ref.im*s.im) >> 31 */
{ return (uint32_t)so_w32((int64_t)ref.re * x.re + (int64_t)ref.im * x.im) >> 31; }

/* ---- TSFDSync::Process (sfd_sync.hpp:76-126) with the short-preamble rule of sora_rx11b_set_preamble (mode 1): symbols up to and including the one that sets
 * rxrate_state or an error -> symbols consumed */
uint32_t st11b_sfd_sync(const so_c16* in, uint32_t n, int mode, st_sfd* s)
{
    uint32_t used = 0;
    while (used < n && s->rxrate_state == RATE_SYNC && s->error_code == 0) {
        const so_c16 x = in[used++];
        const uint32_t bit = dot_sign(s->last_symbol, x);
        s->last_symbol = x;
        s->byte_reg &= 0x7F;
        const uint32_t sbit = (bit ^ s->byte_reg ^ (s->byte_reg >> 3)) & 1;
        s->byte_reg = ((s->byte_reg >> 1) | (bit << 6)) & 0xFF;
        s->word = ((s->word >> 1) | (sbit << 15)) & 0xFFFF;
        s->sync_cnt++;
        if (!s->bit_one_found && !s->bit_zero_found) {
            if (s->word == 0xFFFF) s->bit_one_found = 1;
            else if (mode >= 1 && s->word == 0x0000 && s->sync_cnt >= 16) s->bit_zero_found = 1;
        } else if (s->bit_one_found) {
            if (s->word == 0xF3A0) s->rxrate_state = RATE_1M;
            else if (s->word != 0xFFFF) {
                if (s->bit_err_cnt++ > 32) { s->error_code = E_SFD_FAIL; continue; }
            }
        } else {
            if (s->word == 0x05CF) s->rxrate_state = RATE_2M;
            else if (s->word != 0x0000) {
                if (s->bit_err_cnt++ > 32) { s->error_code = E_SFD_FAIL; continue; }
            }
        }
        if (s->sync_cnt > 128 + 16) s->error_code = E_SFD_TIMEOUT;
    }
    return used;
}

/* ---- TDBPSKDemap::DemapDBPSK (barkerspread.hpp:312-390), TDQPSKDemap::DemapDQPSK (:396-454) */
void st11b_dbpsk_demap(const so_c16* in, uint32_t n, st_stream* s, uint8_t* out)
{
    for (uint32_t b = 0; b < n; b++) {
        uint8_t r = 0; so_c16 ref = s->last_symbol;
        for (int i = 0; i < 8; i++) { r |= (uint8_t)(dot_sign(ref, in[8 * b + i]) << i); ref = in[8 * b + i]; }
        s->last_symbol = ref; out[b] = r;
    }
}
void st11b_dqpsk_demap(const so_c16* in, uint32_t n, st_stream* s, uint8_t* out)
{
    for (uint32_t b = 0; b < n; b++) {
        uint8_t r = 0; so_c16 ref = s->last_symbol;
        for (int i = 0; i < 4; i++) {
            const so_c16 x = in[4 * b + i];
            const int32_t re = so_w32((int64_t)ref.re * x.re + (int64_t)ref.im * x.im);
            const int32_t im = so_w32((int64_t)ref.re * x.im - (int64_t)ref.im * x.re);
            r |= (uint8_t)(((uint32_t)so_w32((int64_t)re + im) >> 31) << (2 * i));
            r |= (uint8_t)(((uint32_t)so_w32((int64_t)re - im) >> 31) << (2 * i + 1));
            ref = x;
        }
        s->last_symbol = ref; out[b] = r;
    }
}

/* ---- CCK (cck.hpp) */
typedef struct { int32_t re, im; } c32_t;
static inline c32_t c32(int32_t re, int32_t im) { c32_t r; r.re = re; r.im = im; return r; }
static inline c32_t c32_add(c32_t a, c32_t b) { return c32(so_w32((int64_t)a.re + b.re), so_w32((int64_t)a.im + b.im)); }
static inline c32_t c32_sra2(c32_t a) { return c32(a.re >> 2, a.im >> 2); }
static inline c32_t c32_rot(c32_t a, int k)
{ switch (k & 3) { case 0: return a; case 1: return c32(-a.im, a.re); case 2: return c32(-a.re, -a.im); default: return c32(a.im, -a.re); } }
static inline c32_t c32_of(so_c16 a) { return c32(a.re, a.im); }
static inline int32_t neg32(int32_t a) { return so_w32(-(int64_t)a); }

/* A1 = P1 + r P0, A2 = r P2 - P3, A3 = P5 + r P4, A4 = P7 - r P6 with r = (-j)^m (cck.hpp:268-275, 392-399, 514-521, 635-642; 81-88, 103-110) */
static void cck_partial(const so_c16 P[8], int m, c32_t A[4])
{
    const int k = (4 - m) & 3;
    A[0] = c32_add(c32_of(P[1]), c32_rot(c32_of(P[0]), k));
    A[1] = c32_add(c32_rot(c32_of(P[2]), k), c32_rot(c32_of(P[3]), 2));
    A[2] = c32_add(c32_of(P[5]), c32_rot(c32_of(P[4]), k));
    A[3] = c32_add(c32_of(P[7]), c32_rot(c32_of(P[6]), k + 2));
}

/* one "Module" of CCK11_DECODER (e.g. cck.hpp:277-390) */
static void cck11_module(const c32_t A[4], int32_t* max_out, uint8_t* val_out)
{
    static const uint8_t base_of[4] = { 0x00, 0x30, 0x10, 0x20 };
    int32_t M[4]; uint8_t V[4];
    for (int s = 0; s < 4; s++) {
        const c32_t bx = c32_sra2(c32_add(A[1], c32_rot(A[0], s))), by = c32_sra2(c32_add(A[3], c32_rot(A[2], s)));
        const int32_t lre = so_w32((int64_t)so_w32((int64_t)bx.re * by.re) + so_w32((int64_t)bx.im * by.im));
        const int32_t lim = so_w32((int64_t)so_w32((int64_t)bx.re * by.im) - so_w32((int64_t)bx.im * by.re));
        const int32_t a1 = lre < 0 ? neg32(lre) : lre, a2 = lim < 0 ? neg32(lim) : lim;
        if (a1 > a2) { if (lre > 0) { M[s] = lre; V[s] = base_of[s] | 0x00; } else { M[s] = neg32(lre); V[s] = base_of[s] | 0x40; } }
        else         { if (lim > 0) { M[s] = lim; V[s] = base_of[s] | 0xC0; } else { M[s] = neg32(lim); V[s] = base_of[s] | 0x80; } }
    }
    int32_t mm; uint8_t vv;
    if (M[0] > M[1]) { mm = M[0]; vv = V[0]; } else { mm = M[1]; vv = V[1]; }
    if (M[2] > M[3]) { if (M[2] > mm) { mm = M[2]; vv = V[2]; } } else { if (M[3] > mm) { mm = M[3]; vv = V[3]; } }
    *max_out = mm; *val_out = vv;
}

static inline void cck_dqpsk_bits(uint8_t* r, int pos, so_c16 ref, so_c16 x)                    /* demap_dqpsk_bits, core/inc/soradsp.h:190-198 */
{
    int32_t re = so_w32((int64_t)ref.re * x.re + (int64_t)ref.im * x.im), im = so_w32((int64_t)ref.re * x.im - (int64_t)ref.im * x.re);
    re >>= 1; im >>= 1;
    *r |= (uint8_t)(((uint32_t)so_w32((int64_t)re + im) >> 31) << pos);
    *r |= (uint8_t)(((uint32_t)so_w32((int64_t)re - im) >> 31) << (pos + 1));
}

/* ---- TCCK11Decoder::CCK11_DECODER (cck.hpp:255-763): the pruned search */
void st11b_cck11_decode(const so_c16* in, uint32_t n, st_stream* s, uint8_t* out_bytes)
{
    for (uint32_t b = 0; b < n; b++) {
        const so_c16* P = in + 8 * (size_t)b;
        c32_t A[4]; int32_t m1, m2, m34; uint8_t v1, v2, v34, out;
        cck_partial(P, 0, A); cck11_module(A, &m1, &v1);
        cck_partial(P, 1, A); cck11_module(A, &m2, &v2); v2 |= 0x08;
        if (m1 > m2) { cck_partial(P, 3, A); cck11_module(A, &m34, &v34); v34 |= 0x0C; out = m1 > m34 ? v1 : v34; }
        else         { cck_partial(P, 2, A); cck11_module(A, &m34, &v34); v34 |= 0x04; out = m2 > m34 ? v2 : v34; }
        cck_dqpsk_bits(&out, 0, s->last_symbol, P[7]);
        out ^= (uint8_t)((s->is_even << 1) | s->is_even);
        s->is_even ^= 1;
        s->last_symbol = P[7];
        out_bytes[b] = out;
    }
}

static int32_t cck5_metric(const so_c16 P[8], int m, int* neg)            /* one half byte of TCCK5P5Decoder (cck.hpp:70-206) */
{
    c32_t A[4]; cck_partial(P, m, A);
    c32_t b0 = c32_add(A[0], A[1]), b1 = c32_add(A[2], A[3]);
    b0.im = neg32(b0.im);
    b0 = c32_sra2(b0); b1 = c32_sra2(b1);
    const int32_t lre = so_w32((int64_t)so_w32((int64_t)b0.re * b1.re) - so_w32((int64_t)b0.im * b1.im));
    *neg = !(lre > 0);
    return lre > 0 ? lre : neg32(lre);
}

/* ---- TCCK5P5Decoder::Process: b_isEven is a local, so every byte is even + odd */
void st11b_cck5p5_decode(const so_c16* in, uint32_t n, st_stream* s, uint8_t* out_bytes)
{
    for (uint32_t b = 0; b < n; b++) {
        uint8_t out = 0;
        for (int half = 0; half < 2; half++) {
            const so_c16* Q = in + 16 * (size_t)b + 8 * half; int n1, n2;
            const int32_t max1 = cck5_metric(Q, 1, &n1), max2 = cck5_metric(Q, 3, &n2);
            const uint8_t nib = max1 > max2 ? (uint8_t)(n1 ? 0x08 : 0x00) : (uint8_t)(n2 ? 0x0C : 0x04);
            if (half == 0) out = nib; else out |= (uint8_t)(nib << 4);
            cck_dqpsk_bits(&out, 4 * half, s->last_symbol, Q[7]);
            if (half == 1) out ^= 0x30;
            s->last_symbol = Q[7];
        }
        out_bytes[b] = out;
    }
}

/* ---- TDesc741 (scramble.hpp:93-170): z^-7 + z^-4 + 1, self-synchronising, bit by bit */
void st11b_desc741(const uint8_t* in, uint32_t n, st_stream* s, uint8_t* out)
{
    for (uint32_t i = 0; i < n; i++) {
        uint8_t x = in[i], st = s->byte_reg & 0x7F, o = 0;
        for (int k = 0; k < 8; k++) {
            uint8_t o1 = (uint8_t)((x ^ st ^ (st >> 3)) & 1);
            st = (uint8_t)((st >> 1) | ((x & 1) << 6));
            o = (uint8_t)((o >> 1) | (o1 << 7));
            x >>= 1;
        }
        s->byte_reg = (uint8_t)(in[i] >> 1);
        out[i] = o;
    }
}

static uint16_t crc16_ccitt(const uint8_t* p, int n)                       /* CalcCRC16, core/inc/CRC16.h: reflected 0x8408, init 0xFFFF, ~ */
{
    uint16_t c = 0xFFFF;
    for (int i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (uint16_t)((c & 1) ? (c >> 1) ^ 0x8408 : c >> 1);
    }
    return (uint16_t)~c;
}

/* ---- TBB11bPlcpParser (PHY_11b.hpp:524-640); a failed CRC leaves the record's other fields 0; an unknown SIGNAL leaves rxrate_state 0 (the brick: unchanged) */
void st11b_plcp_parse(const uint8_t h[6], st_plcp* r)
{
    memset(r, 0, sizeof(*r));
    const uint16_t crc = (uint16_t)(h[4] | (h[5] << 8));
    if (crc16_ccitt(h, 4) != crc) { r->error_code = E_PLCP_HEADER_FAIL; return; }
    const uint8_t signal = h[0], service = h[1];
    uint16_t len = (uint16_t)(h[2] | (h[3] << 8));
    switch (signal) {
    case 0x0A: r->data_rate_kbps = 1000;  len = (uint16_t)(len >> 3); break;
    case 0x14: r->data_rate_kbps = 2000;  len = (uint16_t)(len >> 2); break;
    case 0x37: r->data_rate_kbps = 5500;  len = (uint16_t)(((len * 11) >> 4) - (service >> 7) - ((service >> 3) & 1)); break;
    case 0x6E: r->data_rate_kbps = 11000; len = (uint16_t)(((len * 11) >> 3) - (service >> 7) - ((service >> 3) & 1)); break;
    default:   r->data_rate_kbps = 0;     len = 0;
    }
    r->frame_length = len;
    switch (r->data_rate_kbps) {
    case 1000:  r->rxrate_state = RATE_1M; break;
    case 2000:  r->rxrate_state = RATE_2M; break;
    case 5500:  r->rxrate_state = RATE_5P5M; break;
    case 11000: r->rxrate_state = RATE_11M; break;
    }
}

/* ---- TBB11bFrameSink (PHY_11b.hpp:643-749) fed bytes[0 .. frame_length - 2] into a zeroed 4096-byte buffer: byte frame_length - 1 is never read */
void st11b_frame_sink(const uint8_t* bytes, uint32_t frame_length_in, st_sink* r)
{
    static uint8_t frame_buf[4096];
    const uint32_t frame_buf_size = sizeof(frame_buf);
    const uint16_t frame_length = (uint16_t)frame_length_in;
    uint32_t byte_count = 0, crc32 = 0xFFFFFFFFu;
    memset(r, 0, sizeof(*r));
    if (frame_length < 4) return;                                           /* (uint)(frame_length - 4) is huge: every byte feeds the CRC, nothing is ever decided */
    memset(frame_buf, 0, sizeof(frame_buf));
    for (uint32_t i = 0; i + 1 < frame_length; i++) {
        const uint8_t b = bytes[i];
        if (byte_count < (uint32_t)(int32_t)(frame_length - 4)) {
            if (byte_count < frame_buf_size) frame_buf[byte_count] = b;
            byte_count++;
            crc32 = so_g_crc_lut[(crc32 ^ b) & 0xFF] ^ (crc32 >> 8);
        } else if (byte_count < (uint32_t)frame_length) {
            if (byte_count < frame_buf_size) frame_buf[byte_count] = b;
            byte_count++;
            if (byte_count == (uint32_t)frame_length - 1) {
                uint32_t p = 0;
                for (int k = 0; k < 4; k++)
                    p |= (uint32_t)(byte_count - 3 + k < frame_buf_size ? frame_buf[byte_count - 3 + k] : 0) << (8 * k);
                r->frame_crc32 = p;
                r->error_code = ((~crc32 & 0x00FFFFFFu) == (p & 0x00FFFFFFu)) ? E_FRAME_OK : E_CRC32_FAIL;
            }
        }
    }
}
