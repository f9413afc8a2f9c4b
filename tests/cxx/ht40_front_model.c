/* TEST INFRASTRUCTURE -- the front end of the 40 MHz HT receiver (k_scan_ht40: sora_ht40_process_captures_dev up to the Ht40Found records) as an integer model:
 * what tests/test_gpu_ht40_front.py compares sora_ht40_found_of with, field for field.
 *
 * The walk is oracle/so_rx11n.c's (source calls of 28 raw samples, TDownSample2's queue, RxSwitch, TCCA11n with its time-out reset, the L-LTF into
 * so_cfo_est11n / so_freq_comp11n / so_fft64 / so_siso_est11n, three SIG symbols through so_siso_comp11n / so_mrc11n / so_sig_demap11n and the SIG decoder, the
 * flush at the end of the capture, RxThread's bookkeeping), restated as tests/cxx/rx11n_ext_model.c restates it; every stage is the oracle library's exported,
 * reference-pinned function.  What include/sora_hip.h (sora_ht40_process_captures_dev, sora_ht40_found) and DESIGN.md section 7 g1 state as the front end's own
 * definitions are three switches, so that with all three off this file is so_rx11n_capture, event for event (tests/test_ht40_front_model_cpu.py):
 *   HT40_OWN_SIGN   kept sample m of the capture is x[2m], negated with int16 saturation when m is odd (m counts from the capture's first sample);
 *   HT40_OWN_GATE   the gate is ok && 8 <= mcs <= 14 && cbw40 && 4 <= ht_len <= 4000, on fields parsed HERE from so_sig_decode11n's decoded bytes (which it
 *                   returns also when its own parser refuses); off: so_sig_decode11n's verdict and fields (MCS 8..10, 1500 bytes, the CBW bit not looked at);
 *   HT40_OWN_EVENTS a frame with a sound header is an event (error_code 0: recorded) only if HT-STF, both HT-LTFs and all nsym data symbols lie inside the real
 *                   samples -- nsym = ceil((16 + 8 ht_len + 6) / N_DBPS), N_DBPS = 108 N_BPSC R per stream, twice that with HT40_JOINT -- and nothing of its
 *                   data field is looked at; otherwise no event and the capture is over.  A capture that ends inside the SIG field decodes zero-filled missing
 *                   symbols as flush_graph does.  Off: the reference's rule (the data field decoded, T11aViterbi's padded last burst at a flush).
 * end_sample and the next origin follow so_rx11n_capture's source-call rule in every mode.
 * Linked against nothing: the oracle library is loaded first, with global symbols (tests/ht40_front_model.py).  This file never reads the library under test. */
#include <stdlib.h>
#include <string.h>
#include "so_oracle.h"

enum { HT40_OWN_SIGN = 1, HT40_OWN_GATE = 2, HT40_OWN_EVENTS = 4, HT40_JOINT = 8 };

typedef struct {
    uint32_t a20;           /* kept samples of the capture in front of the position behind the last SIG symbol taken (a recorded frame: its first HT-STF sample) */
    uint32_t mcs, ht_len;   /* 0 for a header that failed */
    uint32_t nsym;          /* own event rule: data symbols of a recorded frame, else 0 */
    int32_t  cfo;           /* as so_cfo_est11n leaves it: phase step per kept sample, 65536 = 2 pi */
    uint32_t end_sample;    /* source position (raw samples) at which the event is seen */
    uint32_t error_code;    /* own event rule: 0 = recorded; else what so_rx11n_capture reports */
    uint32_t pad;
    int64_t  S;             /* sum over both chains and the 52 occupied carriers of |Y1 - Y2|^2, Y1 / Y2 the two L-LTF symbols' so_fft64 outputs */
} ht40_front_event;

/* ------------------------------------------------------------------ TCCA11n (cca_11n.hpp:25-170) on so_autocorr11n_burst, as rx11n_ext_model.c has it */
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

/* ------------------------------------------------------------------ the SIG fields, parsed here */
static unsigned crc8_htsig34(uint64_t ht)                                   /* x^8 + x^2 + x + 1 over HT-SIG bits 0..33, ones' complement (IEEE 802.11n 20.3.9.4.4) */
{
    unsigned crc = 0xFF;
    for (int b = 0; b < 34; b++) { crc ^= (unsigned)(ht >> b) & 1u; crc = (crc & 1u) ? (crc >> 1) ^ 0xE0u : crc >> 1; }
    return (~crc) & 0xFFu;
}

/* why a header is refused, in the parser's order (0: its front is sound and the gate takes it) */
enum { SIG_OK = 0, SIG_LSIG_BITS, SIG_LSIG_PARITY, SIG_LSIG_RATE, SIG_LSIG_LENGTH, SIG_HT_CRC, SIG_MCS_LOW, SIG_MCS_HIGH, SIG_CBW20, SIG_LEN_SHORT, SIG_LEN_LONG, SIG_CAUSES };

typedef struct { int cause; uint32_t rate_code, parity_ok, lsig_len, crc_ok, mcs, cbw40, ht_len; } sig_t;

static void parse_sig(const uint8_t out9[9], sig_t* s)
{
    const uint32_t sig = (uint32_t)out9[0] | (uint32_t)out9[1] << 8 | (uint32_t)out9[2] << 16;
    uint64_t ht = 0;
    for (int i = 0; i < 6; i++) ht |= (uint64_t)out9[3 + i] << (8 * i);
    memset(s, 0, sizeof(*s));
    s->rate_code = sig & 0xF; s->parity_ok = !(__builtin_popcount(sig) & 1); s->lsig_len = ((sig >> 5) & 0xFFF) * 2;
    s->crc_ok = crc8_htsig34(ht) == (unsigned)((ht >> 34) & 0x3FFF);           /* the CRC, and the six tail bits behind it zero */
    s->mcs = (uint32_t)ht & 0x7F; s->cbw40 = (uint32_t)(ht >> 7) & 1; s->ht_len = (uint32_t)(ht >> 8) & 0xFFFF;
    s->cause = (sig & 0xFC0010) ? SIG_LSIG_BITS : !s->parity_ok ? SIG_LSIG_PARITY : s->rate_code < 8 ? SIG_LSIG_RATE : s->lsig_len > 1500 ? SIG_LSIG_LENGTH
             : !s->crc_ok ? SIG_HT_CRC : s->mcs < 8 ? SIG_MCS_LOW : s->mcs > 14 ? SIG_MCS_HIGH : !s->cbw40 ? SIG_CBW20 : s->ht_len < 4 ? SIG_LEN_SHORT
             : s->ht_len > 4000 ? SIG_LEN_LONG : SIG_OK;
}

static uint32_t nbpsc_of(uint32_t mcs) { return mcs == 8 ? 1u : mcs <= 10 ? 2u : mcs <= 12 ? 4u : 6u; }
static uint32_t rate_of(uint32_t mcs) { return (mcs == 10 || mcs == 12 || mcs == 14) ? SO_CR_34 : mcs == 13 ? SO_CR_23 : SO_CR_12; }
static uint32_t ht40_nsym(uint32_t mcs, uint32_t len, int joint)
{
    const uint32_t cr = rate_of(mcs), nd = (108u * nbpsc_of(mcs) * (cr == SO_CR_12 ? 1u : cr == SO_CR_23 ? 2u : 3u) / (cr == SO_CR_12 ? 2u : cr == SO_CR_23 ? 3u : 4u)) << (joint ? 1 : 0);
    return (16u + 8u * len + 6u + nd - 1u) / nd;
}

/* counters over everything walked since the last ht40_front_reset_counters() */
static struct {
    int sig_fields;                 /* SIG fields decoded */
    int disagreements;              /* ... on which the extraction here and so_sig_decode11n differ where that accepts (or it refuses what the reference's gate takes here) */
    int ref_accepts_cbw40;          /* ... that so_sig_decode11n accepts with the CBW bit set: T11nSigParser does not look at it */
    int cause[SIG_CAUSES];          /* own gate: headers by verdict */
    int flush_nsig[3];              /* captures that ended after 0, 1, 2 whole-or-padded SIG symbols with the L-LTF taken (own event rule) */
    int cut_frames;                 /* own event rule: sound headers whose frame the capture cuts off */
    int timeouts;                   /* carrier-sense time-outs */
} g_n;
void ht40_front_reset_counters(void) { memset(&g_n, 0, sizeof(g_n)); }
void ht40_front_counters(int out[8 + SIG_CAUSES])
{
    out[0] = g_n.sig_fields; out[1] = g_n.disagreements; out[2] = g_n.ref_accepts_cbw40; out[3] = g_n.flush_nsig[0]; out[4] = g_n.flush_nsig[1];
    out[5] = g_n.flush_nsig[2]; out[6] = g_n.cut_frames; out[7] = g_n.timeouts;
    for (int k = 0; k < SIG_CAUSES; k++) out[8 + k] = g_n.cause[k];
}

/* ------------------------------------------------------------------ the graph */
enum { SYM_L_LTF = 1, SYM_SIG, SYM_HT_STF, SYM_HT_LTF, SYM_DATA };

typedef struct {
    cca_t cca; int flags;
    uint32_t error_code; int recorded; int cca_detected; int symbol_type;
    int16_t vfo[24];
    so_c16 ch[2][64];
    so_c16 h[2][128], hinv[2][128];
    uint16_t remain_symbols; uint32_t mcs, ht_length, code_rate, nsym;
    so_c16 lq[2][128]; int ln;
    so_c16 fq[2][8]; int fn;
    so_c16 sq[2][80]; int sn;
    so_c16 sig[192]; int nsig;
    so_c16 ltf[2][128]; int nltf;
    uint8_t* soft; uint32_t soft_n, soft_cap;
    uint32_t frame_crc;
    uint32_t pos;                   /* kept samples pushed so far, counted from the capture's first */
    uint32_t a20; int32_t cfo; int64_t S;
} rx_t;

static void frame_reset(rx_t* rx)
{
    rx->error_code = SO_E_SUCCESS; rx->recorded = 0; rx->cca_detected = 0; rx->symbol_type = SYM_L_LTF;
    rx->remain_symbols = 0;
    cca_reset(&rx->cca);
    rx->ln = rx->fn = rx->sn = rx->nsig = rx->nltf = 0; rx->soft_n = 0;
    rx->mcs = rx->ht_length = rx->nsym = 0;
}

static void soft_push(rx_t* rx, const uint8_t* p, uint32_t n)
{
    if (rx->soft_n + n > rx->soft_cap) { rx->soft_cap = (rx->soft_n + n) * 2 + 1024; rx->soft = (uint8_t*)realloc(rx->soft, rx->soft_cap); }
    memcpy(rx->soft + rx->soft_n, p, n); rx->soft_n += n;
}

/* T11nSigDemap's three symbols -> the SIG decoder -> the gate; 1: a frame follows.  flushed: the end of the capture zero-filled the missing symbols */
static int sig_decode(rx_t* rx, int flushed)
{
    uint8_t soft[144], out9[9]; uint32_t f[9]; sig_t s;
    so_sig_demap11n(rx->sig, soft);
    const int ref_ok = so_sig_decode11n(soft, out9, f) != 0;
    parse_sig(out9, &s);
    g_n.sig_fields++;
    {
        /* wherever the reference's parser accepts, the fields extracted here are its fields; and it accepts exactly what passes the front here at its own gate */
        static const uint32_t kbps[16] = { 0, 0, 0, 0, 0, 0, 0, 0, 48000, 24000, 12000, 6000, 54000, 36000, 18000, 9000 };
        const int front = s.cause == SIG_OK || s.cause >= SIG_MCS_LOW;
        const int own10 = front && s.mcs >= 8 && s.mcs <= 10 && s.ht_len <= 1500;
        if (own10 != ref_ok) g_n.disagreements++;
        else if (ref_ok && (f[1] != kbps[s.rate_code] || !s.parity_ok || !s.crc_ok || f[3] != s.mcs || f[4] != s.ht_len || f[5] != rate_of(s.mcs))) g_n.disagreements++;
        if (ref_ok && s.cbw40) g_n.ref_accepts_cbw40++;
    }
    int ok;
    if (rx->flags & HT40_OWN_GATE) {
        ok = s.cause == SIG_OK;
        g_n.cause[s.cause]++;
        if (ok) { rx->mcs = s.mcs; rx->ht_length = s.ht_len; rx->code_rate = rate_of(s.mcs); }
    } else {
        ok = ref_ok;
        if (ok) { rx->mcs = f[3]; rx->ht_length = f[4]; rx->code_rate = f[5]; }
    }
    if (!ok) { rx->error_code = SO_E_PLCP_HEADER_FAIL; return 0; }
    if (rx->flags & HT40_OWN_EVENTS) {
        rx->nsym = ht40_nsym(rx->mcs, rx->ht_length, rx->flags & HT40_JOINT);
        rx->remain_symbols = (uint16_t)(rx->nsym + 4);                         /* this symbol, HT-STF, two HT-LTFs, the data symbols */
    } else if (rx->flags & HT40_OWN_GATE) {
        static const int ndbps[7] = { 52, 104, 156, 208, 312, 416, 468 };      /* the 20 MHz data field the reference's rule decodes */
        rx->remain_symbols = (uint16_t)(((int)rx->ht_length * 8 + 22 + ndbps[rx->mcs - 8] - 1) / ndbps[rx->mcs - 8] + 4);
    } else rx->remain_symbols = (uint16_t)f[7];
    if (flushed) return 0;                                                     /* a sound header behind a flush: the capture is over, nothing follows */
    return 1;
}

static void decode_frame(rx_t* rx, const uint8_t* soft, uint32_t n, int need_all)
{
    uint8_t* dec = (uint8_t*)malloc((size_t)rx->ht_length + 64);
    uint8_t* mpdu = (uint8_t*)malloc((size_t)rx->ht_length + 8);
    const int got = so_viterbi_frame_ex(soft, n, (int)rx->code_rate, rx->ht_length, dec, 192, 36);
    if (!need_all || got == (int)rx->ht_length + 2) rx->error_code = so_desc_sink(dec, rx->ht_length, mpdu, &rx->frame_crc);
    free(dec); free(mpdu);
}

static void ofdm_symbol(rx_t* rx)
{
    so_c16 y0[64], y1[64];
    if ((rx->flags & HT40_OWN_EVENTS) && rx->symbol_type != SYM_SIG) {         /* behind a sound header only the symbols' places count */
        if (--rx->remain_symbols == 0) rx->recorded = 1;
        return;
    }
    so_fft64(rx->sq[0] + 16, y0); so_fft64(rx->sq[1] + 16, y1);
    switch (rx->symbol_type) {
    case SYM_SIG: {
        so_c16 x0[64], x1[64];
        so_siso_comp11n((const so_c16 (*)[64])rx->ch, y0, y1, x0, x1);
        so_mrc11n(x0, x1, rx->sig + 64 * rx->nsig);
        rx->a20 = rx->pos;
        if (++rx->nsig == 3) { rx->nsig = 0; if (sig_decode(rx, 0)) rx->symbol_type = SYM_HT_STF; }
        break; }
    case SYM_HT_STF: rx->symbol_type = SYM_HT_LTF; break;
    case SYM_HT_LTF:
        memcpy(rx->ltf[0] + 64 * rx->nltf, y0, sizeof(y0)); memcpy(rx->ltf[1] + 64 * rx->nltf, y1, sizeof(y1));
        if (++rx->nltf == 2) { rx->nltf = 0; so_mimo_est11n(rx->ltf[0], rx->ltf[1], rx->h, rx->hinv); rx->symbol_type = SYM_DATA; }
        break;
    default: {
        if (rx->error_code != SO_E_SUCCESS) break;
        so_c16 x0[64], x1[64];
        const int nb = (int)nbpsc_of(rx->mcs);
        const int s = nb >= 4 ? nb / 2 : 1;
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
        if (rx->sn == 80) { rx->sn = 0; ofdm_symbol(rx); }
    }
}

static void flush_graph(rx_t* rx)
{
    static const so_c16 z[4] = { {0, 0}, {0, 0}, {0, 0}, {0, 0} };
    if (!rx->cca_detected) return;
    if (rx->symbol_type == SYM_L_LTF) { while (rx->ln) push_burst(rx, z, z); if ((rx->flags & HT40_OWN_EVENTS) && rx->symbol_type == SYM_SIG) g_n.flush_nsig[0]++; return; }
    if (rx->fn) push_burst(rx, z, z);
    while (rx->sn) push_burst(rx, z, z);
    if ((rx->flags & HT40_OWN_EVENTS) && rx->symbol_type > SYM_SIG) { g_n.cut_frames++; return; }      /* the padding completed the SIG field: a frame cut off */
    switch (rx->symbol_type) {
    case SYM_SIG:
        if ((rx->flags & HT40_OWN_EVENTS) && rx->error_code == SO_E_SUCCESS) g_n.flush_nsig[rx->nsig]++;
        if (rx->nsig) {
            memset(rx->sig + 64 * rx->nsig, 0, (size_t)(3 - rx->nsig) * 64 * sizeof(so_c16)); rx->nsig = 0;
            if (!sig_decode(rx, 1) && rx->error_code == SO_E_SUCCESS && (rx->flags & HT40_OWN_EVENTS)) g_n.cut_frames++;
        }
        break;
    case SYM_DATA:
        if (rx->error_code == SO_E_SUCCESS && rx->soft_n % 312) {
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

static so_c16 neg_sat(so_c16 v)
{
    so_c16 o; o.re = v.re == INT16_MIN ? INT16_MAX : (int16_t)-v.re; o.im = v.im == INT16_MIN ? INT16_MAX : (int16_t)-v.im;
    return o;
}

/* iq0 / iq1: the two RX chains at 40 MHz, nsamples each, a whole number of 28-sample source bursts.  Writes up to max_ev events and returns how many the capture
 * raised. */
int ht40_front_capture(const so_c16* iq0, const so_c16* iq1, uint32_t nsamples, int flags, ht40_front_event* ev, int max_ev)
{
    static const so_c16 zero = { 0, 0 };
    if (nsamples % 28) return -1;
    rx_t* rx = (rx_t*)calloc(1, sizeof(rx_t));
    rx->flags = flags;
    rx->cca.core = calloc(1, so_autocorr11n_size()); so_autocorr11n_reset(rx->cca.core);
    for (int i = 0; i < 64; i++) rx->cca.his_e[i] = INT64_MAX;
    frame_reset(rx);
    /* the source: the raw samples, those at 2m with m odd negated (the odd raw samples are never looked at: TDownSample2 keeps the even ones) */
    so_c16* x[2];
    const so_c16* in[2] = { iq0, iq1 };
    for (int c = 0; c < 2; c++) {
        x[c] = (so_c16*)malloc(((size_t)nsamples + 1) * sizeof(so_c16));
        memcpy(x[c], in[c], (size_t)nsamples * sizeof(so_c16));
        if (flags & HT40_OWN_SIGN) for (uint32_t i = 2; i < nsamples; i += 4) x[c][i] = neg_sat(x[c][i]);
    }
    so_c16 q[2][56]; memset(q, 0, sizeof(q));
    uint32_t w = 0, r = 0, src = 0, remain = nsamples;
    int ret = 1, nev = 0;
    while (ret) {
        if (remain > 28) { memcpy(q[0] + w, x[0] + src, 28 * sizeof(so_c16)); memcpy(q[1] + w, x[1] + src, 28 * sizeof(so_c16)); w += 28; src += 28; remain -= 28; }
        else if (remain == 0) {
            ret = 0;
            if ((flags & HT40_OWN_EVENTS) && rx->symbol_type > SYM_SIG) g_n.cut_frames++;     /* a sound header whose frame runs past the real samples: no event */
            else {
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
                if (rx->recorded) break;                                       /* (own event rule) the frame's last burst: nothing behind it is looked at before the event */
            }
        const uint32_t err = rx->error_code;
        if (err != SO_E_SUCCESS || rx->recorded) {
            if (err == SO_E_CS_TIMEOUT) { rx->error_code = SO_E_SUCCESS; cca_reset(&rx->cca); g_n.timeouts++; }
            else {
                if (nev < max_ev) {
                    ht40_front_event* f = &ev[nev];
                    memset(f, 0, sizeof(*f));
                    f->error_code = rx->recorded ? 0u : err; f->end_sample = src; f->a20 = rx->a20; f->cfo = rx->cfo; f->S = rx->S;
                    if (err != SO_E_PLCP_HEADER_FAIL) { f->mcs = rx->mcs; f->ht_len = rx->ht_length; f->nsym = rx->nsym; }
                }
                nev++;
                w = r = 0;
                frame_reset(rx);
                rx->pos = src / 2;
            }
        }
    }
    free(rx->soft); free(rx->cca.core); free(x[0]); free(x[1]); free(rx);
    return nev;
}
