/* viterbi56_model.c -- T11aViterbi<.., DEPTH, LOOK>::Process as oracle/so_rx11a.c::so_viterbi_frame_ex restates it, with a FOURTH puncture pattern: rate 5/6
 * (code_rate 3; include/sora_hip.h, SORA_CR_56: per 5 input bits the coded bits A1 B1 A2 B3 A4 B5).  The reference has no decoder for that rate, so this file is the
 * definition the library's k_viterbi56_11n is held to.  It restates the few functions involved (acs, normalize, argmin_state, traceback, the frame loop) and adds
 *   - the branch itself: a puncture group is 6 soft values and 5 trellis steps of kinds (A,B) (A) (B) (A) (B);
 *   - ONE changed rule, for that branch only: the metrics are normalised after every step whose index is a multiple of 8, also INSIDE a group (the reference's rule,
 *     (trellis_index & 7) == 0 after a group, would fire every 40 steps: up to 8 x 84 units of growth in an 8-bit wrapping metric, which decodes nothing);
 * everything else -- metric initialisation, tie-breaks, the arg-min key, the 6-bit prefix, cnt / look / remain of the trace-back schedule (examined after every
 * group) -- is so_viterbi_frame_ex's.  Rates 0..2 are kept beside it so that a test can hold this restatement to the oracle byte for byte
 * (tests/test_viterbi56_model_cpu.py).  Soft values short of a whole group at the end of the stream are not decoded.  Links against nothing. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int parity7(int v) { v ^= v >> 4; v ^= v >> 2; v ^= v >> 1; return v & 1; }
static uint8_t g_cA[64][2], g_cB[64][2];
static int g_init;
static void vit_init(void)
{
    if (g_init) return;
    for (int n = 0; n < 64; n++) for (int br = 0; br < 2; br++) {
        int r = (br << 6) | n;
        g_cA[n][br] = (uint8_t)parity7(r & 0155); g_cB[n][br] = (uint8_t)parity7(r & 0117);
    }
    g_init = 1;
}
static inline uint8_t bm(uint8_t soft, int bit) { soft &= 7; return (uint8_t)(bit ? 2 * (7 - soft) : 2 * soft); }

/* one ACS step; which: 0 = (A,B), 1 = A only, 2 = B only.  Returns the 64 decision bits. */
static uint64_t acs(uint8_t m[64], int which, uint8_t sa, uint8_t sb)
{
    uint8_t nm[64]; uint64_t dec = 0;
    for (int n = 0; n < 64; n++) {
        uint8_t c0 = m[n >> 1], c1 = m[32 + (n >> 1)];
        if (which != 2) { c0 = (uint8_t)(c0 + bm(sa, g_cA[n][0])); c1 = (uint8_t)(c1 + bm(sa, g_cA[n][1])); }
        if (which != 1) { c0 = (uint8_t)(c0 + bm(sb, g_cB[n][0])); c1 = (uint8_t)(c1 + bm(sb, g_cB[n][1])); }
        c0 &= 0xFE; c1 |= 0x01;
        nm[n] = c0 < c1 ? c0 : c1;
        dec |= (uint64_t)(nm[n] & 1) << n;
    }
    memcpy(m, nm, 64);
    return dec;
}
static void normalize(uint8_t m[64])
{
    uint8_t mn = 255;
    for (int n = 0; n < 64; n++) if (m[n] < mn) mn = m[n];
    mn &= 0xFE;
    for (int n = 0; n < 64; n++) m[n] = (uint8_t)(m[n] - mn);
}
static int argmin_state(const uint8_t m[64])
{
    int best = 0; uint32_t bk = 0xFFFFFFFFu;
    for (int n = 0; n < 64; n++) { uint32_t k = ((uint32_t)m[n] << 8) | ((uint32_t)n << 2); if (k < bk) { bk = k; best = n; } }
    return best;
}
static void traceback(const uint64_t* dec, uint32_t cur, const uint8_t m[64], uint8_t* out, uint32_t bits, uint32_t lookahead)
{
    int st = argmin_state(m);
    int pos = st | ((m[st] & 1) << 6);
    uint32_t col = cur;
    for (uint32_t i = 0; i < lookahead; i++) {
        col--; pos = (pos >> 1) & 0x3F;
        pos |= (int)((dec[col] >> pos) & 1) << 6;
    }
    uint8_t* po = out + (bits >> 3);
    for (uint32_t i = 0; i < bits >> 3; i++) {
        uint8_t oc = 0;
        for (int j = 0; j < 8; j++) {
            oc = (uint8_t)((oc << 1) | ((pos >> 6) & 1));
            col--; pos = (pos >> 1) & 0x3F;
            pos |= (int)((dec[col] >> pos) & 1) << 6;
        }
        *--po = oc;
    }
}

/* one step of the 5/6 branch: the step, then the changed rule */
static void step56(uint8_t m[64], uint64_t* dec, uint32_t* tr, int which, uint8_t sa, uint8_t sb)
{
    dec[*tr + 1] = acs(m, which, sa, sb);
    *tr += 1;
    if ((*tr & 7) == 0) normalize(m);
}

/* code_rate 0 = 1/2, 1 = 2/3, 2 = 3/4 (so_viterbi_frame_ex), 3 = 5/6.  -> bytes written to out (frame_length + 2 for a whole frame) */
int v56_viterbi_frame(const uint8_t* soft, uint32_t nsoft, int code_rate, uint32_t frame_length, uint8_t* out, uint32_t DEPTH, uint32_t LOOK)
{
    vit_init();
    const uint32_t PREFIX = 6;
    const uint32_t gb = code_rate == 0 ? 2 : code_rate == 1 ? 3 : code_rate == 2 ? 4 : 6;
    uint64_t* dec = (uint64_t*)malloc(((size_t)nsoft + 8) * sizeof(uint64_t));
    uint8_t m[64];
    for (int n = 0; n < 64; n++) m[n] = 0x30;
    m[0] = 0;
    dec[0] = 0; for (int n = 0; n < 64; n++) dec[0] |= (uint64_t)(m[n] & 1) << n;
    uint32_t tr = 0, ob = 0; int nout = 0;
    const uint8_t* p = soft; const uint8_t* end = soft + nsoft;
    const uint32_t tr_end = frame_length * 8 + 16 + PREFIX;
    while (p + gb <= end) {
        if (code_rate == 3) {
            step56(m, dec, &tr, 0, p[0], p[1]); step56(m, dec, &tr, 1, p[2], 0); step56(m, dec, &tr, 2, 0, p[3]);
            step56(m, dec, &tr, 1, p[4], 0); step56(m, dec, &tr, 2, 0, p[5]);
            p += 6;
        } else {
            if (code_rate == 0)      { dec[tr + 1] = acs(m, 0, p[0], p[1]); tr += 1; p += 2; }
            else if (code_rate == 2) { dec[tr + 1] = acs(m, 0, p[0], p[1]); dec[tr + 2] = acs(m, 1, p[2], 0); dec[tr + 3] = acs(m, 2, 0, p[3]); tr += 3; p += 4; }
            else                     { dec[tr + 1] = acs(m, 0, p[0], p[1]); dec[tr + 2] = acs(m, 1, p[2], 0); tr += 2; p += 3; }
            if ((tr & 7) == 0) normalize(m);
        }
        uint32_t cnt = 0, look = 0;
        if (tr >= tr_end) { cnt = tr_end - ob - PREFIX; look = tr - tr_end; }
        else if (tr >= ob + DEPTH + LOOK + PREFIX) { uint32_t remain = (tr - (ob + DEPTH + LOOK + PREFIX)) % 8; cnt = DEPTH; look = LOOK + remain; }
        if (cnt) {
            uint8_t* buf = (uint8_t*)malloc((cnt >> 3) + 1);
            traceback(dec, tr, m, buf, cnt, look); memcpy(out + nout, buf, cnt >> 3); free(buf);
            ob += cnt; nout += (int)(cnt >> 3);
            if (tr >= tr_end) break;
        }
    }
    free(dec);
    return nout;
}

/* The matching encoder, for tests that want clean streams: nbits input bits (one per byte) from the all-zero state -> the punctured coded bits (one per byte);
 * returns their number.  Whole puncture groups only: nbits is rounded DOWN to a multiple of the group's steps. */
int v56_encode(const uint8_t* bits, uint32_t nbits, int code_rate, uint8_t* coded)
{
    const uint32_t gs = code_rate == 0 ? 1 : code_rate == 1 ? 2 : code_rate == 2 ? 3 : 5;
    int n = 0; int state = 0;
    for (uint32_t t = 0; t + gs <= nbits; t += gs)
        for (uint32_t i = 0; i < gs; i++) {
            const int br = state >> 5, ns = ((state & 31) << 1) | (bits[t + i] & 1), r = (br << 6) | ns;
            const uint8_t a = (uint8_t)parity7(r & 0155), b = (uint8_t)parity7(r & 0117);
            state = ns;
            /* 1/2: A B; 2/3: A1 B1 A2; 3/4: A1 B1 A2 B3; 5/6: A1 B1 A2 B3 A4 B5 */
            const int keepA = i == 0 || (i & 1), keepB = i == 0 || !(i & 1);
            if (keepA) coded[n++] = a;
            if (keepB) coded[n++] = b;
        }
    return n;
}
