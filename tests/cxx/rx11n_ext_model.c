/* TEST INFRASTRUCTURE -- the 802.11n 2x2 receive graph with T11nSigParser's MCS gate moved (sora_rx11n_set_mcs_max): what the GPU rows are compared with
 * when the gate stands above 10, where no compiled reference decodes a frame.
 *
 * The walk is oracle/so_rx11n.c's (source calls of 28 raw samples, TDownSample2, RxSwitch, the symbol state machine with remain_symbols, the flush at
 * the end of the capture, RxThread's bookkeeping), restated; every stage is the oracle library's exported, reference-pinned function: so_autocorr11n_burst
 * (under TCCA11n's peak counter), so_cfo_est11n, so_freq_comp11n, so_fft64, so_siso_est11n / _comp11n, so_mrc11n, so_sig_demap11n, so_sig_decode11n,
 * so_mimo_est11n / _comp11n, so_pilot_track11n, so_demap11n, so_deinterleave11n, so_viterbi_frame_ex(.., 192, 36), so_desc_sink.  Three things are this file's own:
 *   - the SIG fields are parsed here from so_sig_decode11n's decoded bytes (which it returns also when its parser refuses): T11nSigParser's checks in its
 *     order, with the one comparison `mcs >= 11` replaced by `mcs > mcs_max`; the coding rate of MCS 11..14 (1/2, 3/4, 2/3, 3/4) and N_DBPS = 208, 312,
 *     416, 468 continue the tables the parser reads for MCS 8..10;
 *   - rate_selector's branches for MCS 11..14 (fb11ndemod_config.hpp:136-147): N_BPSC 4 / 6 through so_demap11n and so_deinterleave11n;
 *   - TStreamJoin<2, 52 nb> -> TStreamConcat<2, s> with s = 1, 1, 2, 3: joined position g takes element (g / 2s) s + g % s of stream (g / s) & 1.
 * With mcs_max = 10 this is so_rx11n_capture, event for event (tests/test_rx11n_mcs_cpu.py).  Linked against nothing: the oracle library is loaded first,
 * with global symbols (tests/rx11n_ext_model.py). */
#include <stdlib.h>
#include <string.h>
#include "so_oracle.h"

/* ------------------------------------------------------------------ TCCA11n (cca_11n.hpp:25-170) on so_autocorr11n_burst */
typedef struct {
    void* core;
    int64_t his_e[64]; int his_index;
    int peak_found, peak_count; uint32_t sense_count;
} cca_t;

static void cca_reset(cca_t* c) { c->sense_count = 0; c->peak_found = 0; c->peak_count = 0; }

static int cca_burst(cca_t* c, const so_c16 x0[4], const so_c16 x1[4], int* timeout)
{
    int64_t acorr[4], energy[4];
    int detected = 0;
    so_autocorr11n_burst(c->core, x0, x1, acorr, energy);
    for (int i = 0; i < 4; i++) {
        const int64_t den = (int64_t)((uint64_t)c->his_e[c->his_index] + 1u);
        const int64_t eb = (den == -1 && energy[i] == INT64_MIN) ? 0 : energy[i] / (den == 0 ? 1 : den);
        if (!c->peak_found) {
            c->sense_count += 1;
            if (eb > 5 && acorr[i] > (energy[i] >> 1)) { c->sense_count = 0; c->peak_count++; c->peak_found = 1; }
            else c->peak_count = 0;
        } else if (acorr[i] < (energy[i] >> 3)) {
            const int good = c->peak_count > 96 && c->peak_count < 160;
            c->peak_found = 0; c->peak_count = 0;
            if (good) { detected = 1; break; }
        } else {
            c->peak_count++;
            if (c->peak_count > 160) { c->peak_found = 0; c->peak_count = 0; }
        }
        c->his_e[c->his_index++] = energy[i];
        c->his_index %= 64;
    }
    *timeout = (c->sense_count >= 84 && !detected);
    return detected;
}

/* ------------------------------------------------------------------ the SIG parser with the gate at mcs_max */
static unsigned crc8_htsig34(uint64_t ht)                                   /* x^8 + x^2 + x + 1 over HT-SIG bits 0..33, ones' complement (IEEE 802.11n 20.3.9.4.4) */
{
    unsigned crc = 0xFF;
    for (int b = 0; b < 34; b++) { crc ^= (unsigned)(ht >> b) & 1u; crc = (crc & 1u) ? (crc >> 1) ^ 0xE0u : crc >> 1; }
    return (~crc) & 0xFFu;
}

typedef struct { uint32_t mcs, ht_length, code_rate, remain; } sig_t;

static int parse_sig(const uint8_t out9[9], int mcs_max, sig_t* s)
{
    static const int ndbps[7] = { 52, 104, 156, 208, 312, 416, 468 };          /* N_DBPS of MCS 8..14, 20 MHz, long guard interval */
    const uint32_t sig = (uint32_t)out9[0] | (uint32_t)out9[1] << 8 | (uint32_t)out9[2] << 16;
    uint64_t ht = 0;
    for (int i = 0; i < 6; i++) ht |= (uint64_t)out9[3 + i] << (8 * i);
    if (sig & 0xFC0010) return 0;                                              /* L-SIG: tail and reserved bit */
    if (__builtin_popcount(sig) & 1) return 0;                                 /* parity */
    if ((sig & 0xF) < 8) return 0;                                             /* no 802.11a rate */
    if (((sig >> 5) & 0xFFF) * 2 > 1500) return 0;
    if (crc8_htsig34(ht) != (unsigned)((ht >> 34) & 0x3FFF)) return 0;         /* the CRC, and the six tail bits behind it zero */
    const uint32_t mcs = (uint32_t)ht & 0x7F;
    if (mcs < 8 || mcs > (uint32_t)mcs_max) return 0;                          /* THE comparison: mcs >= 11 in PHY_11n.hpp:497 */
    const uint32_t len = (uint32_t)(ht >> 8) & 0xFFFF;
    if (len > 1500) return 0;
    s->mcs = mcs; s->ht_length = len;
    s->code_rate = (mcs == 10 || mcs == 12 || mcs == 14) ? SO_CR_34 : mcs == 13 ? SO_CR_23 : SO_CR_12;
    const int bits = (int)len * 8 + 16 + 6, nd = ndbps[mcs - 8];
    s->remain = (uint32_t)((bits + nd - 1) / nd + 4);
    return 1;
}

static int g_parser_disagreements;                                             /* SIG fields on which this parser and so_sig_decode11n differ below the gate of 10 */
int rx11n_ext_parser_disagreements(void) { return g_parser_disagreements; }

/* ------------------------------------------------------------------ the graph */
enum { SYM_L_LTF = 1, SYM_SIG, SYM_HT_STF, SYM_HT_LTF, SYM_DATA };

typedef struct {
    cca_t cca; int mcs_max;
    uint32_t error_code; int cca_detected; int symbol_type;
    int16_t vfo[24];
    so_c16 ch[2][64];
    so_c16 h[2][128], hinv[2][128];
    uint16_t remain_symbols; uint32_t mcs, ht_length, code_rate;
    so_c16 lq[2][128]; int ln;
    so_c16 fq[2][8]; int fn;
    so_c16 sq[2][80]; int sn;
    so_c16 sig[192]; int nsig;
    so_c16 ltf[2][128]; int nltf;
    uint8_t* soft; uint32_t soft_n, soft_cap;
    uint32_t frame_crc;
    so_frame_result* res; int nres, max_res;
    uint8_t* mpdu_buf; uint32_t mpdu_used, mpdu_cap;
} rx_t;

static void frame_reset(rx_t* rx)
{
    rx->error_code = SO_E_SUCCESS; rx->cca_detected = 0; rx->symbol_type = SYM_L_LTF;
    rx->remain_symbols = 0;
    cca_reset(&rx->cca);
    rx->ln = rx->fn = rx->sn = rx->nsig = rx->nltf = 0; rx->soft_n = 0;
}

static void soft_push(rx_t* rx, const uint8_t* p, uint32_t n)
{
    if (rx->soft_n + n > rx->soft_cap) { rx->soft_cap = (rx->soft_n + n) * 2 + 1024; rx->soft = (uint8_t*)realloc(rx->soft, rx->soft_cap); }
    memcpy(rx->soft + rx->soft_n, p, n); rx->soft_n += n;
}

static int sig_decode(rx_t* rx)                                               /* T11nSigDemap's three symbols -> the parser; 1: a frame follows */
{
    uint8_t soft[144], out9[9]; uint32_t fields[9]; sig_t s;
    so_sig_demap11n(rx->sig, soft);
    const int ref_ok = so_sig_decode11n(soft, out9, fields);
    const int ok = parse_sig(out9, rx->mcs_max, &s);
    {                                                                          /* at the reference's gate the two parsers are one */
        sig_t t; const int ok10 = parse_sig(out9, 10, &t);
        if (ok10 != (ref_ok != 0) || (ok10 && (t.mcs != fields[3] || t.ht_length != fields[4] || t.code_rate != fields[5] || t.remain != fields[7]))) g_parser_disagreements++;
    }
    if (!ok) { rx->error_code = SO_E_PLCP_HEADER_FAIL; return 0; }
    rx->mcs = s.mcs; rx->ht_length = s.ht_length; rx->code_rate = s.code_rate; rx->remain_symbols = (uint16_t)s.remain;
    return 1;
}

static void decode_frame(rx_t* rx, const uint8_t* soft, uint32_t n, int need_all)
{
    uint8_t* dec = (uint8_t*)malloc((size_t)rx->ht_length + 64);
    uint8_t* tmp = NULL; uint8_t* mpdu = rx->mpdu_buf + rx->mpdu_used;
    if (rx->mpdu_used + rx->ht_length > rx->mpdu_cap) { tmp = (uint8_t*)malloc((size_t)rx->ht_length + 8); mpdu = tmp; }
    const int got = so_viterbi_frame_ex(soft, n, (int)rx->code_rate, rx->ht_length, dec, 192, 36);
    if (!need_all || got == (int)rx->ht_length + 2) rx->error_code = so_desc_sink(dec, rx->ht_length, mpdu, &rx->frame_crc);
    free(dec); free(tmp);
}

static void ofdm_symbol(rx_t* rx)
{
    so_c16 y0[64], y1[64];
    so_fft64(rx->sq[0] + 16, y0); so_fft64(rx->sq[1] + 16, y1);
    switch (rx->symbol_type) {
    case SYM_SIG: {
        so_c16 x0[64], x1[64];
        so_siso_comp11n((const so_c16 (*)[64])rx->ch, y0, y1, x0, x1);
        so_mrc11n(x0, x1, rx->sig + 64 * rx->nsig);
        if (++rx->nsig == 3) { rx->nsig = 0; if (sig_decode(rx)) rx->symbol_type = SYM_HT_STF; }
        break; }
    case SYM_HT_STF: rx->symbol_type = SYM_HT_LTF; break;
    case SYM_HT_LTF:
        memcpy(rx->ltf[0] + 64 * rx->nltf, y0, sizeof(y0)); memcpy(rx->ltf[1] + 64 * rx->nltf, y1, sizeof(y1));
        if (++rx->nltf == 2) { rx->nltf = 0; so_mimo_est11n(rx->ltf[0], rx->ltf[1], rx->h, rx->hinv); rx->symbol_type = SYM_DATA; }
        break;
    default: {
        if (rx->error_code != SO_E_SUCCESS) break;
        so_c16 x0[64], x1[64];
        const int nb = rx->mcs == 8 ? 1 : rx->mcs <= 10 ? 2 : rx->mcs <= 12 ? 4 : 6;      /* rate_selector */
        const int s = nb >= 4 ? nb / 2 : 1;                                                /* TStreamConcat<2, s> */
        uint8_t s0[312], s1[312], d[2][312], joined[624];
        so_mimo_comp11n((const so_c16 (*)[128])rx->hinv, y0, y1, x0, x1);
        so_pilot_track11n(rx->vfo + 16, x0, x1);
        so_demap11n(nb, x0, s0); so_deinterleave11n(nb, 0, s0, d[0]);
        so_demap11n(nb, x1, s1); so_deinterleave11n(nb, 1, s1, d[1]);
        for (int g = 0; g < 104 * nb; g++) joined[g] = d[(g / s) & 1][g / (2 * s) * s + g % s];
        soft_push(rx, joined, (uint32_t)(104 * nb));
        break; }
    }
    rx->remain_symbols--;
    if (rx->remain_symbols == 0 && rx->error_code == SO_E_SUCCESS) decode_frame(rx, rx->soft, rx->soft_n, 0);
}

static void push_burst(rx_t* rx, const so_c16 x0[4], const so_c16 x1[4])
{
    if (!rx->cca_detected) {
        int to;
        if (cca_burst(&rx->cca, x0, x1, &to)) rx->cca_detected = 1;
        else if (to && rx->error_code == SO_E_SUCCESS) rx->error_code = SO_E_CS_TIMEOUT;
        return;
    }
    if (rx->symbol_type == SYM_L_LTF) {
        memcpy(rx->lq[0] + rx->ln, x0, 16); memcpy(rx->lq[1] + rx->ln, x1, 16); rx->ln += 4;
        if (rx->ln == 128) {
            so_c16 c0[128], c1[128], l0[128], l1[128];
            rx->ln = 0;
            so_cfo_est11n(rx->lq[0], rx->lq[1], rx->vfo);
            so_freq_comp11n(rx->vfo, rx->lq[0], rx->lq[1], c0, c1, 16);
            so_fft64(c0, l0); so_fft64(c0 + 64, l0 + 64); so_fft64(c1, l1); so_fft64(c1 + 64, l1 + 64);
            so_siso_est11n(l0, l1, rx->ch);
            rx->symbol_type = SYM_SIG;
        }
        return;
    }
    memcpy(rx->fq[0] + rx->fn, x0, 16); memcpy(rx->fq[1] + rx->fn, x1, 16); rx->fn += 4;
    if (rx->fn == 8) {
        rx->fn = 0;
        so_freq_comp11n(rx->vfo, rx->fq[0], rx->fq[1], rx->sq[0] + rx->sn, rx->sq[1] + rx->sn, 1);
        rx->sn += 8;
        if (rx->sn == 80) { rx->sn = 0; ofdm_symbol(rx); }
    }
}

static void flush_graph(rx_t* rx)
{
    static const so_c16 z[4] = { {0, 0}, {0, 0}, {0, 0}, {0, 0} };
    if (!rx->cca_detected) return;
    if (rx->symbol_type == SYM_L_LTF) { while (rx->ln) push_burst(rx, z, z); return; }
    if (rx->fn) push_burst(rx, z, z);
    while (rx->sn) push_burst(rx, z, z);
    switch (rx->symbol_type) {
    case SYM_SIG:
        if (rx->nsig) {
            memset(rx->sig + 64 * rx->nsig, 0, (size_t)(3 - rx->nsig) * 64 * sizeof(so_c16)); rx->nsig = 0;
            (void)sig_decode(rx);
        }
        break;
    case SYM_DATA:
        if (rx->error_code == SO_E_SUCCESS && rx->soft_n % 312) {              /* T11aViterbi's input burst, padded with zero soft values */
            const uint32_t n = (rx->soft_n + 311) / 312 * 312;
            uint8_t* padded = (uint8_t*)calloc(n, 1);
            memcpy(padded, rx->soft, rx->soft_n);
            decode_frame(rx, padded, n, 1);
            free(padded);
        }
        break;
    default: break;
    }
}

int rx11n_ext_capture(const so_c16* iq0, const so_c16* iq1, uint32_t nsamples, int mcs_max, so_frame_result* res, int max_res, uint8_t* mpdu_buf, uint32_t mpdu_cap)
{
    static const so_c16 zero = { 0, 0 };
    rx_t* rx = (rx_t*)calloc(1, sizeof(rx_t));
    rx->mcs_max = mcs_max; rx->res = res; rx->max_res = max_res; rx->mpdu_buf = mpdu_buf; rx->mpdu_cap = mpdu_cap;
    rx->cca.core = calloc(1, so_autocorr11n_size()); so_autocorr11n_reset(rx->cca.core);
    for (int i = 0; i < 64; i++) rx->cca.his_e[i] = INT64_MAX;
    frame_reset(rx);
    so_c16 q[2][56]; memset(q, 0, sizeof(q));
    uint32_t w = 0, r = 0, src = 0, remain = nsamples;
    int ret = 1;
    while (ret) {
        if (remain > 28) { memcpy(q[0] + w, iq0 + src, 28 * sizeof(so_c16)); memcpy(q[1] + w, iq1 + src, 28 * sizeof(so_c16)); w += 28; src += 28; remain -= 28; }
        else if (remain == 0) {
            ret = 0;
            if (w - r) {
                so_c16 a[4], b[4];
                for (int e = 0; e < 4; e++) { const uint32_t i = r + 2 * e; a[e] = i < w ? q[0][i] : zero; b[e] = i < w ? q[1][i] : zero; }
                r = w = 0;
                push_burst(rx, a, b);
            }
            flush_graph(rx);
        }
        else { memcpy(q[0] + w, iq0 + src, remain * sizeof(so_c16)); memcpy(q[1] + w, iq1 + src, remain * sizeof(so_c16)); w += 28; src += remain; remain = 0; }
        if (ret)
            while (w - r >= 8) {
                so_c16 a[4], b[4];
                for (int e = 0; e < 4; e++) { a[e] = q[0][r + 2 * e]; b[e] = q[1][r + 2 * e]; }
                r += 8;
                if (r == w) r = w = 0;
                push_burst(rx, a, b);
            }
        const uint32_t err = rx->error_code;
        if (err != SO_E_SUCCESS) {
            if (err == SO_E_CS_TIMEOUT) { rx->error_code = SO_E_SUCCESS; cca_reset(&rx->cca); }
            else {
                if (rx->nres < rx->max_res) {
                    so_frame_result* f = &rx->res[rx->nres++];
                    memset(f, 0, sizeof(*f));
                    f->error_code = err; f->end_sample = src;
                    if (err != SO_E_PLCP_HEADER_FAIL) {
                        f->rate_kbps = rx->mcs; f->length = (uint16_t)rx->ht_length; f->crc32 = rx->frame_crc; f->mpdu_offset = rx->mpdu_used;
                        if (rx->mpdu_used + rx->ht_length <= rx->mpdu_cap) rx->mpdu_used += rx->ht_length;
                    }
                }
                w = r = 0;
                frame_reset(rx);
            }
        }
    }
    const int n = rx->nres;
    free(rx->soft); free(rx->cca.core); free(rx);
    return n;
}
