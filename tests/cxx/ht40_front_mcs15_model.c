/* TEST INFRASTRUCTURE -- the front end of the 40 MHz HT receiver with the MCS gate as a PARAMETER (sora_ht40_set_mcs_max) as an integer model:
 * what tests/test_gpu_ht40_mcs15.py compares sora_ht40_found_of with, field for field.
 *
 * The walk is tests/cxx/ht40_front_gi_model.c's, statement for statement, with two changes: the gate reads 8 <= MCS <= mcs_max (14 or 15) where that file reads
 * 8 <= MCS <= 14, and the symbol count knows MCS 15 (64-QAM, rate 5/6: N_DBPS 540 per stream, 1080 in the joint coding).  With mcs_max = 14 this file is
 * ht40_front_gi_model.c event for event (tests/test_ht40_mcs15_model_cpu.py).  Linked against nothing: the oracle library is loaded first, with global symbols
 * (tests/ht40_mcs15_model.py).  This file never reads the library under test. */
#include <stdlib.h>
#include <string.h>
#include "so_oracle.h"

enum { HT40_JOINT = 8, HT40_GUARD = 16 };

typedef struct {
    uint32_t a20;           /* kept samples of the capture in front of the position behind the last SIG symbol taken (a recorded frame: its first HT-STF sample) */
    uint32_t mcs, ht_len;   /* 0 for a header that failed */
    uint32_t nsym;          /* data symbols of a recorded frame, else 0 */
    int32_t  cfo;           /* as so_cfo_est11n leaves it: phase step per kept sample, 65536 = 2 pi */
    uint32_t end_sample;    /* source position (raw samples) at which the event is seen */
    uint32_t error_code;    /* 0 = recorded; else SO_E_PLCP_HEADER_FAIL */
    uint32_t short_gi;      /* 1: a recorded frame whose header set the Short GI bit, read because of HT40_GUARD */
    int64_t  S;             /* sum over both chains and the 52 occupied carriers of |Y1 - Y2|^2, Y1 / Y2 the two L-LTF symbols' so_fft64 outputs */
} ht40_front_gi_event;

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

/* ------------------------------------------------------------------ the SIG fields, parsed here from so_sig_decode11n's decoded bytes */
static unsigned crc8_htsig34(uint64_t ht)
{
    unsigned crc = 0xFF;
    for (int b = 0; b < 34; b++) { crc ^= (unsigned)(ht >> b) & 1u; crc = (crc & 1u) ? (crc >> 1) ^ 0xE0u : crc >> 1; }
    return (~crc) & 0xFFu;
}

typedef struct { int ok; uint32_t mcs, ht_len, short_gi; } sig_t;

static void parse_sig(const uint8_t out9[9], uint32_t mcs_max, sig_t* s)
{
    const uint32_t sig = (uint32_t)out9[0] | (uint32_t)out9[1] << 8 | (uint32_t)out9[2] << 16;
    uint64_t ht = 0;
    for (int i = 0; i < 6; i++) ht |= (uint64_t)out9[3 + i] << (8 * i);
    const int parity_ok = !(__builtin_popcount(sig) & 1);
    const uint32_t rate_code = sig & 0xF, lsig_len = ((sig >> 5) & 0xFFF) * 2, cbw40 = (uint32_t)(ht >> 7) & 1;
    const int crc_ok = crc8_htsig34(ht) == (unsigned)((ht >> 34) & 0x3FFF);      /* the CRC, and the six tail bits behind it zero */
    s->mcs = (uint32_t)ht & 0x7F; s->ht_len = (uint32_t)(ht >> 8) & 0xFFFF;
    s->short_gi = (uint32_t)(ht >> 31) & 1;                                       /* HT-SIG bit 31; the CRC covers it */
    s->ok = !(sig & 0xFC0010) && parity_ok && rate_code >= 8 && lsig_len <= 1500 && crc_ok && s->mcs >= 8 && s->mcs <= mcs_max && cbw40 && s->ht_len >= 4 && s->ht_len <= 4000;
}

static uint32_t nbpsc_of(uint32_t mcs) { return mcs == 8 ? 1u : mcs <= 10 ? 2u : mcs <= 12 ? 4u : 6u; }
static uint32_t ht40_nsym(uint32_t mcs, uint32_t len, int joint)
{
    const uint32_t num = mcs == 15 ? 5u : (mcs == 10 || mcs == 12 || mcs == 14) ? 3u : mcs == 13 ? 2u : 1u, den = num + 1u;
    const uint32_t nd = (108u * nbpsc_of(mcs) * num / den) << (joint ? 1 : 0);
    return (16u + 8u * len + 6u + nd - 1u) / nd;
}

/* ------------------------------------------------------------------ the graph */
enum { SYM_L_LTF = 1, SYM_SIG, SYM_FRAME };

typedef struct {
    cca_t cca; int flags; uint32_t mcs_max;
    uint32_t error_code; int recorded; int cca_detected; int symbol_type;
    int16_t vfo[24];
    so_c16 ch[2][64];
    uint32_t remain_symbols, mcs, ht_length, nsym, short_gi;
    int sym_len;                    /* kept samples of the symbol being gathered: 80; 72 for the data symbols of a short-GI frame */
    so_c16 lq[2][128]; int ln;
    so_c16 fq[2][8]; int fn;
    so_c16 sq[2][80]; int sn;
    so_c16 sig[192]; int nsig;
    uint32_t pos;                   /* kept samples pushed so far, counted from the capture's first */
    uint32_t a20; int32_t cfo; int64_t S;
} rx_t;

static void frame_reset(rx_t* rx)
{
    rx->error_code = SO_E_SUCCESS; rx->recorded = 0; rx->cca_detected = 0; rx->symbol_type = SYM_L_LTF;
    rx->remain_symbols = 0; rx->sym_len = 80;
    cca_reset(&rx->cca);
    rx->ln = rx->fn = rx->sn = rx->nsig = 0;
    rx->mcs = rx->ht_length = rx->nsym = rx->short_gi = 0;
}

/* T11nSigDemap's three symbols -> the SIG decoder -> the gate; 1: a frame follows.  flushed: the end of the capture zero-filled the missing symbols */
static int sig_decode(rx_t* rx, int flushed)
{
    uint8_t soft[144], out9[9]; uint32_t f[9]; sig_t s;
    so_sig_demap11n(rx->sig, soft);
    (void)so_sig_decode11n(soft, out9, f);                                        /* (its decoded bytes are returned also when its own parser refuses) */
    parse_sig(out9, rx->mcs_max, &s);
    if (!s.ok) { rx->error_code = SO_E_PLCP_HEADER_FAIL; return 0; }
    rx->mcs = s.mcs; rx->ht_length = s.ht_len;
    rx->short_gi = (rx->flags & HT40_GUARD) ? s.short_gi : 0u;
    rx->nsym = ht40_nsym(rx->mcs, rx->ht_length, rx->flags & HT40_JOINT);
    rx->remain_symbols = rx->nsym + 4;                                            /* this symbol, HT-STF, two HT-LTFs, the data symbols */
    return !flushed;                                                              /* a sound header behind a flush: the capture is over, nothing follows */
}

static void ofdm_symbol(rx_t* rx)
{
    if (rx->symbol_type == SYM_FRAME) {                                           /* behind a sound header only the symbols' places count */
        if (--rx->remain_symbols == 0) rx->recorded = 1;
        else if (rx->short_gi && rx->remain_symbols <= rx->nsym) rx->sym_len = 72;   /* HT-STF and both HT-LTFs are behind: the data symbols of a short-GI frame */
        return;
    }
    so_c16 y0[64], y1[64], x0[64], x1[64];
    so_fft64(rx->sq[0] + 16, y0); so_fft64(rx->sq[1] + 16, y1);
    so_siso_comp11n((const so_c16 (*)[64])rx->ch, y0, y1, x0, x1);
    so_mrc11n(x0, x1, rx->sig + 64 * rx->nsig);
    rx->a20 = rx->pos;
    if (++rx->nsig == 3) { rx->nsig = 0; if (sig_decode(rx, 0)) rx->symbol_type = SYM_FRAME; }
    rx->remain_symbols--;
}

static void push_burst(rx_t* rx, const so_c16 x0[4], const so_c16 x1[4])
{
    rx->pos += 4;
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
            rx->cfo = so_cfo_est11n(rx->lq[0], rx->lq[1], rx->vfo);
            so_freq_comp11n(rx->vfo, rx->lq[0], rx->lq[1], c0, c1, 16);
            so_fft64(c0, l0); so_fft64(c0 + 64, l0 + 64); so_fft64(c1, l1); so_fft64(c1 + 64, l1 + 64);
            rx->S = 0;
            for (int k = 1; k < 64; k++) {
                if (k >= 27 && k < 38) continue;                               /* the 52 occupied carriers: bins 1..26 and 38..63 */
                const so_c16* l[2] = { l0, l1 };
                for (int r = 0; r < 2; r++) {
                    const int64_t dr = (int64_t)l[r][k].re - l[r][64 + k].re, di = (int64_t)l[r][k].im - l[r][64 + k].im;
                    rx->S += dr * dr + di * di;
                }
            }
            so_siso_est11n(l0, l1, rx->ch);
            rx->symbol_type = SYM_SIG;
            rx->a20 = rx->pos;
        }
        return;
    }
    memcpy(rx->fq[0] + rx->fn, x0, 16); memcpy(rx->fq[1] + rx->fn, x1, 16); rx->fn += 4;
    if (rx->fn == 8) {
        rx->fn = 0;
        so_freq_comp11n(rx->vfo, rx->fq[0], rx->fq[1], rx->sq[0] + rx->sn, rx->sq[1] + rx->sn, 1);
        rx->sn += 8;
        if (rx->sn == rx->sym_len) { rx->sn = 0; ofdm_symbol(rx); }
    }
}

static void flush_graph(rx_t* rx)
{
    static const so_c16 z[4] = { {0, 0}, {0, 0}, {0, 0}, {0, 0} };
    if (!rx->cca_detected) return;
    if (rx->symbol_type == SYM_L_LTF) { while (rx->ln) push_burst(rx, z, z); return; }
    if (rx->fn) push_burst(rx, z, z);
    while (rx->sn) push_burst(rx, z, z);
    if (rx->symbol_type != SYM_SIG) return;                                       /* the padding completed the SIG field: a frame cut off */
    if (rx->nsig) {
        memset(rx->sig + 64 * rx->nsig, 0, (size_t)(3 - rx->nsig) * 64 * sizeof(so_c16)); rx->nsig = 0;
        (void)sig_decode(rx, 1);
    }
}

static so_c16 neg_sat(so_c16 v)
{
    so_c16 o; o.re = v.re == INT16_MIN ? INT16_MAX : (int16_t)-v.re; o.im = v.im == INT16_MIN ? INT16_MAX : (int16_t)-v.im;
    return o;
}

/* iq0 / iq1: the two RX chains at 40 MHz, nsamples each, a whole number of 28-sample source bursts.  flags: HT40_JOINT (the joint coding's N_SYM), HT40_GUARD.
 * mcs_max: the gate.  Writes up to max_ev events and returns how many the capture raised. */
int ht40_front_mcs15_capture(const so_c16* iq0, const so_c16* iq1, uint32_t nsamples, int flags, uint32_t mcs_max, ht40_front_gi_event* ev, int max_ev)
{
    static const so_c16 zero = { 0, 0 };
    if (nsamples % 28) return -1;
    rx_t* rx = (rx_t*)calloc(1, sizeof(rx_t));
    rx->flags = flags; rx->mcs_max = mcs_max;
    rx->cca.core = calloc(1, so_autocorr11n_size()); so_autocorr11n_reset(rx->cca.core);
    for (int i = 0; i < 64; i++) rx->cca.his_e[i] = INT64_MAX;
    frame_reset(rx);
    /* the source: the raw samples, those at 2m with m odd negated (the odd raw samples are never looked at: TDownSample2 keeps the even ones) */
    so_c16* x[2];
    const so_c16* in[2] = { iq0, iq1 };
    for (int c = 0; c < 2; c++) {
        x[c] = (so_c16*)malloc(((size_t)nsamples + 1) * sizeof(so_c16));
        memcpy(x[c], in[c], (size_t)nsamples * sizeof(so_c16));
        for (uint32_t i = 2; i < nsamples; i += 4) x[c][i] = neg_sat(x[c][i]);
    }
    so_c16 q[2][56]; memset(q, 0, sizeof(q));
    uint32_t w = 0, r = 0, src = 0, remain = nsamples;
    int ret = 1, nev = 0;
    while (ret) {
        if (remain > 28) { memcpy(q[0] + w, x[0] + src, 28 * sizeof(so_c16)); memcpy(q[1] + w, x[1] + src, 28 * sizeof(so_c16)); w += 28; src += 28; remain -= 28; }
        else if (remain == 0) {
            ret = 0;
            if (rx->symbol_type != SYM_FRAME) {                                /* (a sound header whose frame runs past the real samples: no event) */
                if (w - r) {
                    so_c16 a[4], b[4];
                    for (int e = 0; e < 4; e++) { const uint32_t i = r + 2 * e; a[e] = i < w ? q[0][i] : zero; b[e] = i < w ? q[1][i] : zero; }
                    r = w = 0;
                    push_burst(rx, a, b);
                }
                flush_graph(rx);
            }
        }
        else { memcpy(q[0] + w, x[0] + src, remain * sizeof(so_c16)); memcpy(q[1] + w, x[1] + src, remain * sizeof(so_c16)); w += 28; src += remain; remain = 0; }
        if (ret)
            while (w - r >= 8) {
                so_c16 a[4], b[4];
                for (int e = 0; e < 4; e++) { a[e] = q[0][r + 2 * e]; b[e] = q[1][r + 2 * e]; }
                r += 8;
                if (r == w) r = w = 0;
                push_burst(rx, a, b);
                if (rx->recorded) break;                                       /* the frame's last burst: nothing behind it is looked at before the event */
            }
        const uint32_t err = rx->error_code;
        if (err != SO_E_SUCCESS || rx->recorded) {
            if (err == SO_E_CS_TIMEOUT) { rx->error_code = SO_E_SUCCESS; cca_reset(&rx->cca); }
            else {
                if (nev < max_ev) {
                    ht40_front_gi_event* f = &ev[nev];
                    memset(f, 0, sizeof(*f));
                    f->error_code = rx->recorded ? 0u : err; f->end_sample = src; f->a20 = rx->a20; f->cfo = rx->cfo; f->S = rx->S;
                    if (err != SO_E_PLCP_HEADER_FAIL) { f->mcs = rx->mcs; f->ht_len = rx->ht_length; f->nsym = rx->nsym; f->short_gi = rx->short_gi; }
                }
                nev++;
                w = r = 0;
                frame_reset(rx);
                rx->pos = src / 2;
            }
        }
    }
    free(rx->cca.core); free(x[0]); free(x[1]); free(rx);
    return nev;
}
