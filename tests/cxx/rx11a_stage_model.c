/* rx11a_stage_model.c -- the front-end bricks of the 802.11a receive graph, one by one, in the reference bricks' own form (TEST INFRASTRUCTURE: tests/rx11a_stage_model.py
 * compiles and binds it).  Each function restates ONE brick from its source over the records of include/sora_hip.h as 32-bit words:
 *   TDCRemoveEx<4>::Filter brick/inc/dc.hpp:46-86      TDCEstimator dc.hpp:99-165      TCCA11a Brick11/src/cca.hpp:104-441
 *   T11aViterbiSig viterbi.hpp:8-49 (Viterbi_sig11, viterbicore.h:35-261)               T11aPLCPParser PHY_11a.hpp:518-604
 * The bricks keep rings with an index; the records keep them oldest first, so a ring is loaded with its index at 0 and stored rotated.  The short training symbols'
 * correlation patterns (cca.hpp:268-277) are handed in by the binding. */
#include <stdint.h>
#include <string.h>

typedef struct { int16_t re, im; } c16;
static int16_t w16(int32_t v) { return (int16_t)(uint16_t)(uint32_t)v; }
static int32_t w32(int64_t v) { return (int32_t)(uint32_t)(uint64_t)v; }
static c16 unpack(uint32_t u) { c16 r; r.re = (int16_t)(uint16_t)(u & 0xFFFF); r.im = (int16_t)(uint16_t)(u >> 16); return r; }
static uint32_t pack(c16 a) { return (uint32_t)(uint16_t)a.re | ((uint32_t)(uint16_t)a.im << 16); }
static c16 sra(c16 a, int n) { c16 r; r.re = (int16_t)(a.re >> n); r.im = (int16_t)(a.im >> n); return r; }
static c16 sub16(c16 a, c16 b) { c16 r; r.re = w16((int32_t)a.re - b.re); r.im = w16((int32_t)a.im - b.im); return r; }
static c16 add16(c16 a, c16 b) { c16 r; r.re = w16((int32_t)a.re + b.re); r.im = w16((int32_t)a.im + b.im); return r; }
static int32_t iabs(int32_t v) { return v < 0 ? w32(-(int64_t)v) : v; }
/* conj_mul(vi& re, vi& im, a, b) (vector128.h:1038-1044) */
static void conj_mul(c16 a, c16 b, int32_t* re, int32_t* im)
{
    *re = w32((int64_t)a.re * b.re + (int64_t)a.im * b.im);
    *im = w32((int64_t)w16(-(int32_t)b.im) * a.re + (int64_t)b.re * a.im);
}

enum { CCA_WORDS = 44, DC_WORDS = 4, STOP_ON_TIMEOUT = 1 };
#define E_CS_TIMEOUT 0x80000007u
#define E_PLCP_HEADER_FAIL 0x80000005u
/* branch counters, in the classes of so_cs_counters (oracle/so_oracle.h) */
enum { C_TRUE_TEST, C_EST_LOCK, C_EST_NO_LOCK, C_EST_LOCK_LATE_PEAK, C_LOCK_DROPPED, C_LOCK_DROPPED_DC_UPDATE, C_FRAME_DETECTED, C_PEAK_RAISED, C_DC_UPDATE,
       C_TIMEOUT_RAISED, C_TRUE_TEST_TIMEOUT_PENDING, NCOUNTERS };

static c16 g_pat[16][16];
void st11a_set_pattern(const int16_t* p) { memcpy(g_pat, p, sizeof(g_pat)); }

/* ---- TDCRemoveEx<4> */
void st11a_dc_remove(const uint32_t* in, uint32_t nbursts, uint32_t dc, uint32_t* out)
{
    for (uint32_t i = 0; i < 4 * nbursts; i++) out[i] = pack(sub16(unpack(in[i]), unpack(dc)));
}

/* ---- TDCEstimator: one burst.  -> 1 where DC was updated */
typedef struct { uint32_t update_cnt; c16 sum_dc, dc; } dcest;
static int dcest_burst(dcest* d, const c16 pi[4])
{
    c16 h = { 0, 0 }; int upd = 0;
    for (int e = 0; e < 4; e++) h = add16(h, sra(pi[e], 5));           /* hadd(shift_right(pi, 5)) */
    d->sum_dc = add16(d->sum_dc, h);
    if (d->update_cnt == 0) { d->dc = add16(d->dc, sra(d->sum_dc, 2)); d->update_cnt = 8; d->sum_dc.re = d->sum_dc.im = 0; upd = 1; }
    d->update_cnt--;
    return upd;
}
void st11a_dc_estimate(const uint32_t* in, uint32_t nbursts, uint32_t* st)
{
    dcest d = { st[0], unpack(st[1]), unpack(st[2]) };
    for (uint32_t b = 0; b < nbursts; b++) {
        c16 pi[4]; for (int e = 0; e < 4; e++) pi[e] = unpack(in[4 * b + e]);
        dcest_burst(&d, pi);
    }
    st[0] = d.update_cnt; st[1] = pack(d.sum_dc); st[2] = pack(d.dc);
}

/* ---- TCCA11a */
typedef struct { int32_t e[4]; int idx; int32_t reg; } acc4;                  /* CMovingWindow<int, 4> + CAccumulator (dspalg.hpp:5-98) */
static void acc_push(acc4* a, int32_t d) { a->reg = w32((int64_t)a->reg + d - a->e[a->idx]); a->e[a->idx] = d; a->idx = (a->idx + 1) & 3; }
typedef struct {
    uint32_t cca_state, error_code, thr, reading, ctx_peak_index;
    uint32_t sync, auto_count, sense_count, high_count; int32_t peak_corr, peak_index;
    c16 his[4][4]; int his_idx;
    acc4 ac_re, ac_im, energy;
} cca;
static void cca_load(cca* s, const uint32_t* w)
{
    memset(s, 0, sizeof(*s));
    s->cca_state = w[0]; s->error_code = w[1]; s->thr = w[2]; s->reading = w[3]; s->ctx_peak_index = w[4];
    s->sync = w[5] & 1; s->auto_count = w[6]; s->sense_count = w[7]; s->high_count = w[8]; s->peak_corr = (int32_t)w[9]; s->peak_index = (int32_t)(w[10] & 15);
    for (int g = 0; g < 4; g++) {
        for (int e = 0; e < 4; e++) s->his[g][e] = unpack(w[12 + 4 * g + e]);
        s->ac_re.e[g] = (int32_t)w[28 + g]; s->ac_im.e[g] = (int32_t)w[32 + g]; s->energy.e[g] = (int32_t)w[36 + g];
    }
    s->ac_re.reg = (int32_t)w[40]; s->ac_im.reg = (int32_t)w[41]; s->energy.reg = (int32_t)w[42];
}
static void cca_store(const cca* s, uint32_t* w)
{
    w[0] = s->cca_state; w[1] = s->error_code; w[3] = s->reading; w[4] = s->ctx_peak_index;
    w[5] = s->sync; w[6] = s->auto_count; w[7] = s->sense_count; w[8] = s->high_count; w[9] = (uint32_t)s->peak_corr; w[10] = (uint32_t)s->peak_index;
    for (int g = 0; g < 4; g++) {
        for (int e = 0; e < 4; e++) w[12 + 4 * g + e] = pack(s->his[(s->his_idx + g) & 3][e]);
        w[28 + g] = (uint32_t)s->ac_re.e[(s->ac_re.idx + g) & 3]; w[32 + g] = (uint32_t)s->ac_im.e[(s->ac_im.idx + g) & 3];
        w[36 + g] = (uint32_t)s->energy.e[(s->energy.idx + g) & 3];
    }
    w[40] = (uint32_t)s->ac_re.reg; w[41] = (uint32_t)s->ac_im.reg; w[42] = (uint32_t)s->energy.reg;
}
static int32_t cross_corr(const cca* s, int k, const c16* pattern)             /* GetCrossCorrelation (cca.hpp:202-218) */
{
    int32_t sre[4] = { 0, 0, 0, 0 }, sim[4] = { 0, 0, 0, 0 };
    for (int v = 0; v < 4; v++) {
        for (int e = 0; e < 4; e++) {
            int32_t re, im; conj_mul(pattern[4 * v + e], s->his[k][e], &re, &im);
            sre[e] = w32((int64_t)sre[e] + re); sim[e] = w32((int64_t)sim[e] + im);
        }
        k = (k + 1) & 3;
    }
    return w32((int64_t)iabs(w32((int64_t)sre[0] + sre[1] + sre[2] + sre[3])) + iabs(w32((int64_t)sim[0] + sim[1] + sim[2] + sim[3])));
}
/* one burst of Process (cca.hpp:318-431).  -> 1 where the burst passes the gate; *dropped: a lock was dropped on it */
static int cca_burst(cca* s, const c16 pi[4], uint64_t* cnt, int* dropped)
{
    *dropped = 0;
    if (!s->sync) {
        c16 pii[4]; int32_t sr = 0, si = 0, se = 0;
        for (int e = 0; e < 4; e++) pii[e] = sra(pi[e], 2);
        for (int e = 0; e < 4; e++) {                                            /* GetAutoCorrelation (:165-186), GetEnergy (:188-193) */
            int32_t re, im; conj_mul(pii[e], s->his[s->his_idx][e], &re, &im);
            sr = w32((int64_t)sr + (re >> 4)); si = w32((int64_t)si + (im >> 4));
            se = w32((int64_t)se + (w32((int64_t)pii[e].re * pii[e].re + (int64_t)pii[e].im * pii[e].im) >> 4));
        }
        acc_push(&s->ac_re, sr); acc_push(&s->ac_im, si); acc_push(&s->energy, se);
        const int32_t iAuto = w32((int64_t)iabs(s->ac_re.reg) + iabs(s->ac_im.reg)), iEnergy = s->energy.reg;
        memcpy(s->his[s->his_idx], pii, sizeof(pii)); s->his_idx = (s->his_idx + 1) & 3;
        s->sense_count += 4;
        if (iEnergy > (int32_t)s->thr && iAuto >= iEnergy - (iEnergy >> 3)) {
            s->auto_count++; s->sense_count = 0;
            if (cnt) { cnt[C_TRUE_TEST]++; if (s->error_code == E_CS_TIMEOUT) cnt[C_TRUE_TEST_TIMEOUT_PENDING]++; }
            if (s->auto_count >= 4) {
                int32_t sum_corr = 0;                                            /* establish_sync (:220-243) */
                s->peak_corr = 0;
                for (int i = 0; i < 16; i++) {
                    const int32_t corr = cross_corr(s, s->his_idx, g_pat[i]);
                    if (corr > s->peak_corr) { s->peak_corr = corr; s->peak_index = i; }
                    sum_corr = w32((int64_t)sum_corr + corr);
                }
                if (s->peak_corr > (sum_corr >> 3)) {
                    s->sync = 1; s->reading = (uint32_t)iEnergy; s->high_count = 0;
                    if (cnt) cnt[C_EST_LOCK]++;
                    if (s->peak_index > 3) { s->high_count = (uint32_t)s->peak_index / 4; s->peak_index &= 3; if (cnt) cnt[C_EST_LOCK_LATE_PEAK]++; }
                    s->ctx_peak_index = (uint32_t)s->peak_index;
                } else if (cnt) cnt[C_EST_NO_LOCK]++;
            }
        } else s->auto_count = 0;
    } else {
        for (int e = 0; e < 4; e++) s->his[s->his_idx][e] = sra(pi[e], 2);
        s->his_idx = (s->his_idx + 1) & 3;
        s->high_count++;
        if (s->high_count % 4 == 0) {                                            /* check_sync (:245-265) */
            const int32_t corr = cross_corr(s, s->his_idx, g_pat[s->peak_index]);
            if (corr < (s->peak_corr >> 1)) {
                if (s->high_count > 8) { s->cca_state = 1; if (cnt) cnt[C_FRAME_DETECTED]++; }
                else { s->sync = 0; s->sense_count = 0; *dropped = 1; if (cnt) cnt[C_LOCK_DROPPED]++; }
            } else if (corr > s->peak_corr) { s->peak_corr = corr; if (cnt) cnt[C_PEAK_RAISED]++; }
        }
    }
    return !s->sync;
}
/* the time-out at the end of a burst (:433-437).  -> 1 where it changed error_code */
static int cca_timeout(cca* s, uint64_t* cnt)
{
    if (s->sense_count >= 84 && !s->sync) {
        const int raised = s->error_code != E_CS_TIMEOUT;
        if (raised && cnt) cnt[C_TIMEOUT_RAISED]++;
        s->error_code = E_CS_TIMEOUT;
        return raised;
    }
    return 0;
}

/* TCCA11a alone over DC-removed bursts -> bursts consumed; out / npass: the gated bursts */
uint32_t st11a_cca(const uint32_t* in, uint32_t nbursts, uint32_t flags, uint32_t* st, uint32_t* out, uint32_t* npass, uint64_t* cnt)
{
    cca s; cca_load(&s, st);
    uint32_t used = 0, np = 0;
    while (used < nbursts && s.cca_state != 1) {
        c16 pi[4]; int dropped;
        for (int e = 0; e < 4; e++) pi[e] = unpack(in[4 * used + e]);
        if (cca_burst(&s, pi, cnt, &dropped)) { memcpy(out + 4 * np, in + 4 * used, 16); np++; }
        used++;
        if (cca_timeout(&s, cnt) && (flags & STOP_ON_TIMEOUT)) break;
    }
    cca_store(&s, st); *npass = np;
    return used;
}

/* TDCRemoveEx -> TCCA11a -> TDCEstimator over raw bursts -> bursts consumed */
uint32_t st11a_carrier_sense(const uint32_t* in, uint32_t nbursts, uint32_t flags, uint32_t* st, uint64_t* cnt)
{
    cca s; cca_load(&s, st);
    dcest d = { st[CCA_WORDS], unpack(st[CCA_WORDS + 1]), unpack(st[CCA_WORDS + 2]) };
    uint32_t used = 0;
    while (used < nbursts && s.cca_state != 1) {
        c16 pi[4]; int dropped;
        for (int e = 0; e < 4; e++) pi[e] = sub16(unpack(in[4 * used + e]), d.dc);
        if (cca_burst(&s, pi, cnt, &dropped)) {
            const int upd = dcest_burst(&d, pi);
            if (upd && cnt) { cnt[C_DC_UPDATE]++; if (dropped) cnt[C_LOCK_DROPPED_DC_UPDATE]++; }
        }
        used++;
        if (cca_timeout(&s, cnt) && (flags & STOP_ON_TIMEOUT)) break;
    }
    cca_store(&s, st);
    st[CCA_WORDS] = d.update_cnt; st[CCA_WORDS + 1] = pack(d.sum_dc); st[CCA_WORDS + 2] = pack(d.dc);
    return used;
}

/* ---- The harness around carrier sense: RxThread (fb11a_demod.cpp:29-81) over TMemSamples' source calls, 14 samples at the 20 MHz rate each, bursts of 4 as they
 * fit (oracle/so_rx11a.c:691-768).  x: the capture at the 20 MHz rate, whole source calls.  The carrier-sense entry is called one burst at a time.  A time-out stands
 * until the end of the source call that raised it, then ResetCarrierSense + Reset.  A detection at frame start s is looked up in starts[]: the frame's event is
 * raised in the call that holds the burst ending at ends[] (Flush + Reset: the source's partial burst is dropped, the next burst starts on the call grid); a
 * detection without a row ends the walk.  det[]: the frame starts; pos[] / rec[][48]: the records at the resume points (a burst about to start on the call grid
 * in plain carrier sense).  -> the number of resume points */
static int cs_plain(const uint32_t* st) { return st[0] == 0 && st[1] == 0 && st[5] == 0 && st[6] == 0; }
static void cs_reset(uint32_t* st) { st[0] = st[1] = 0; memset(st + 5, 0, 39 * 4); st[CCA_WORDS] = 8; st[CCA_WORDS + 1] = 0; }
uint32_t st11a_sense_walk(const uint32_t* x, uint32_t n20, uint32_t thr, const uint32_t* starts, const uint32_t* ends, uint32_t nrows, uint32_t* det, uint32_t max_det,
                          uint32_t* ndet, uint32_t* pos, uint32_t* rec, uint32_t cap, uint64_t* cnt)
{
    uint32_t st[CCA_WORDS + DC_WORDS]; memset(st, 0, sizeof(st)); st[2] = thr; st[CCA_WORDS] = 8;
    uint32_t p = 0, np = 0, nd = 0;
    while (p + 4 <= n20) {
        if (p % 14 == 0 && cs_plain(st)) { if (np < cap) { pos[np] = p; memcpy(rec + 48 * (size_t)np, st, sizeof(st)); } np++; }
        st11a_carrier_sense(x + p, 1, 0, st, cnt);
        p += 4;
        if (st[0] == 1) {
            if (nd < max_det) det[nd] = p;
            nd++;
            uint32_t r = 0; while (r < nrows && starts[r] != p) r++;
            if (r == nrows) { p = n20 + 4; break; }
            p = (ends[r] + 13) / 14 * 14;
            cs_reset(st);
            continue;
        }
        if (p + 4 > (p + 13) / 14 * 14 && st[1] == E_CS_TIMEOUT) cs_reset(st);     /* the last burst of its source call */
    }
    if (p == n20 && n20 % 14 == 0 && cs_plain(st)) { if (np < cap) { pos[np] = p; memcpy(rec + 48 * (size_t)np, st, sizeof(st)); } np++; }
    *ndet = nd;
    return np;
}

/* ---- T11aViterbiSig: Viterbi_sig11 (viterbicore.h:35-261) with output_bit = 24, then >> 6 (viterbi.hpp:38-39).  Metrics are bytes; the low bit of a metric is
 * the decision (the even candidate has it cleared, the odd one set: viterbicore.h:310, 315); normalisation every eight steps takes the minimum's even part off. */
static int par7(int v) { v ^= v >> 4; v ^= v >> 2; v ^= v >> 1; return v & 1; }
uint32_t st11a_viterbi_sig(const uint8_t* soft)
{
    uint8_t m[64], nm[64]; uint64_t dec[25];
    for (int n = 0; n < 64; n++) m[n] = 0x30;
    m[0] = 0; dec[0] = 0;
    for (int t = 1; t <= 24; t++) {
        const int sa = soft[2 * (t - 1)], sb = soft[2 * (t - 1) + 1];
        uint64_t d = 0;
        for (int n = 0; n < 64; n++) {
            uint8_t c[2];
            for (int br = 0; br < 2; br++) {
                const int r = (br << 6) | n, a = par7(r & 0155), b = par7(r & 0117);
                c[br] = (uint8_t)(m[32 * br + (n >> 1)] + (a ? 2 * (7 - sa) : 2 * sa) + (b ? 2 * (7 - sb) : 2 * sb));
            }
            c[0] &= 0xFE; c[1] |= 1;
            nm[n] = c[0] < c[1] ? c[0] : c[1];
            d |= (uint64_t)(nm[n] & 1) << n;
        }
        memcpy(m, nm, 64); dec[t] = d;
        if ((t & 7) == 0) {
            uint8_t mn = 255;
            for (int n = 0; n < 64; n++) if (m[n] < mn) mn = m[n];
            for (int n = 0; n < 64; n++) m[n] = (uint8_t)(m[n] - (mn & 0xFE));
        }
    }
    int best = 0; uint32_t bk = 0xFFFFFFFFu;                                     /* smallest metric, then smallest state (viterbicore.h:479-524) */
    for (int n = 0; n < 64; n++) { const uint32_t k = ((uint32_t)m[n] << 8) | ((uint32_t)n << 2); if (k < bk) { bk = k; best = n; } }
    int pos = best | ((m[best] & 1) << 6), col = 24;
    uint32_t v = 0;
    for (int byte = 2; byte >= 0; byte--) {
        uint32_t oc = 0;
        for (int j = 0; j < 8; j++) {
            oc = (oc << 1) | (uint32_t)((pos >> 6) & 1);
            col--; pos = (pos >> 1) & 0x3F; pos |= (int)((dec[col] >> pos) & 1) << 6;
        }
        v |= oc << (8 * byte);
    }
    return v >> 6;
}

/* ---- T11aPLCPParser::_parse_plcp (PHY_11a.hpp:548-580) on a context that starts at 0: rec = error_code, data_rate_kbps, frame_length, code_rate, total_symbols */
void st11a_plcp_parse(uint32_t sig, uint32_t* rec)
{
    static const uint32_t rate[16] = { 0, 0, 0, 0, 0, 0, 0, 0, 48000, 24000, 12000, 6000, 54000, 36000, 18000, 9000 };      /* ieee80211a_cmn.h:97-107 */
    memset(rec, 0, 20); rec[0] = E_PLCP_HEADER_FAIL;
    sig &= 0xFFFFFF;
    if (sig & 0xFC0010) return;
    uint32_t p = (sig >> 16) ^ sig; p = (p >> 8) ^ p; p = (p >> 4) ^ p; p = (p >> 2) ^ p; p = (p >> 1) ^ p;
    if (p & 1) return;
    rec[1] = rate[sig & 0xF];
    if (rec[1] == 0) return;
    switch (rec[1]) {                                                             /* BB11aGetCodingRateFromDataRate: 0 = 1/2, 1 = 2/3, 2 = 3/4 */
    case 48000: rec[3] = 1; break;
    case 9000: case 18000: case 36000: case 54000: rec[3] = 2; break;
    default: rec[3] = 0;
    }
    rec[2] = (sig >> 5) & 0xFFF;
    if (rec[2] > 2500) return;
    uint32_t ndbps = 0;
    switch (rec[1]) { case 6000: ndbps = 24; break; case 9000: ndbps = 36; break; case 12000: ndbps = 48; break; case 18000: ndbps = 72; break;
                      case 24000: ndbps = 96; break; case 36000: ndbps = 144; break; case 48000: ndbps = 192; break; case 54000: ndbps = 216; break; }
    rec[4] = (rec[2] * 8 + 16 + 6 + ndbps - 1) / ndbps + 1;                       /* B11aGetSymbolCount (ieee80211a_cmn.h:151-157), and this symbol */
    rec[0] = 0;
}
