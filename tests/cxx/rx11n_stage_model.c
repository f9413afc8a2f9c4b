/* TEST INFRASTRUCTURE -- the bricks that complete the 802.11n receive graph, one by one and in the reference bricks' own form, over the records of include/sora_hip.h
 * (int32 words): TCCA11n with MimoAutoCorr's product and sum arrays (cca_11n.hpp:25-170, autocorr.hpp:5-147), T11aDesc with its register and byte table
 * (scramble.hpp:269-355) and TBB11aFrameSink byte by byte (PHY_11a.hpp:609-700).  tests/rx11n_stage_model.py compiles and binds it; it links against nothing.
 * The kernels state the same bricks differently (windowed sums by prefix scan, a scrambler phase table, a parallel CRC): that the two agree bit for bit is the test. */
#include <stdint.h>
#include <string.h>

typedef struct { int16_t re, im; } c16;
static int32_t w32(int64_t v) { return (int32_t)(uint32_t)(uint64_t)v; }
static int16_t neg16(int16_t v) { return (int16_t)(-(int32_t)v); }

/* ---- TCCA11n.  state: 264 words (sora_cca11n_state); branch[16] (may be NULL) counts what the walk reached:
 *   0..3 a detection deciding at sample 0..3 of its burst, 4 a fake plateau (a fall with peak_count <= 96 or >= 160), 5 too many peaks (peak_count > 160),
 *   6 time-outs re-armed, 7 a time-out left standing, 8 samples compared against an LLONG_MAX ring entry, 9 samples whose squared norm wrapped 32 bits on a chain
 *   (a -32768 rail; the sums of 32 terms >> 5 cannot wrap),
 *   10 samples of which both chains' energy terms (>> 5) were 0, 11 the call entered with a ring slipped against the bursts (his_index mod 4 != 0) */
enum { W_STATE, W_ERR, W_READING, W_SENSE, W_FOUND, W_COUNT, W_HIS, W_TIMEOUTS, W_RING = 8, W_HIST = 136, W_WORDS = 264 };
#define E_CS_TIMEOUT 0x80000007u
#define FLAG_REARM 1u

uint32_t st11n_cca(const c16* x0, const c16* x1, uint32_t nbursts, uint32_t flags, int32_t* st, uint32_t* branch)
{
    uint32_t* s = (uint32_t*)st;
    uint32_t dummy[16];
    if (!branch) branch = dummy;
    if (s[W_STATE] != 0 || s[W_ERR] != 0 || nbursts == 0) return 0;
    /* MimoAutoCorr as it stands behind the record's 64 samples, from a constructed brick: the products still inside the windows and their sums */
    c16 his[2][32]; int32_t hcr[2][32], hci[2][32], he[2][32], sr[2] = { 0, 0 }, si[2] = { 0, 0 }, se[2] = { 0, 0 };
    for (int r = 0; r < 2; r++)
        for (int k = 0; k < 32; k++) {
            c16 a, b;
            memcpy(&b, &s[W_HIST + 64 * r + k], 4); memcpy(&a, &s[W_HIST + 64 * r + 32 + k], 4);
            his[r][k] = a;
            hcr[r][k] = w32((int64_t)a.re * b.re + (int64_t)a.im * b.im) >> 5;
            hci[r][k] = w32((int64_t)neg16(b.im) * a.re + (int64_t)b.re * a.im) >> 5;
            he[r][k] = w32((int64_t)a.re * a.re + (int64_t)a.im * a.im) >> 5;
            sr[r] = w32((int64_t)sr[r] + hcr[r][k]); si[r] = w32((int64_t)si[r] + hci[r][k]); se[r] = w32((int64_t)se[r] + he[r][k]);
        }
    int idx = 0;                                                 /* slot of the oldest sample; where the window starts in the arrays does not matter */
    int64_t ring[64];
    for (int k = 0; k < 64; k++) ring[k] = (int64_t)(((uint64_t)s[W_RING + 2 * k + 1] << 32) | s[W_RING + 2 * k]);
    uint32_t his_index = s[W_HIS] & 63u, sense = s[W_SENSE], count = s[W_COUNT], used = 0;
    int found = s[W_FOUND] != 0;
    if (his_index & 3u) branch[11]++;
    c16 last[2][64];
    memcpy(last[0], &s[W_HIST], 256); memcpy(last[1], &s[W_HIST + 64], 256);
    while (used < nbursts && s[W_STATE] == 0 && s[W_ERR] == 0) {
        const c16* x[2] = { x0 + 4 * (size_t)used, x1 + 4 * (size_t)used };
        int64_t acorr[4], energy[4];
        int32_t pr[2][4], pi[2][4], pe[2][4];
        int wrapped[4] = { 0, 0, 0, 0 }, silent[4] = { 1, 1, 1, 1 };
        used++;
        for (int r = 0; r < 2; r++)
            for (int j = 0; j < 4; j++) {
                const c16 a = x[r][j], b = his[r][idx + j];
                int32_t cr = w32((int64_t)a.re * b.re + (int64_t)a.im * b.im) >> 5, ci = w32((int64_t)neg16(b.im) * a.re + (int64_t)b.re * a.im) >> 5;
                his[r][idx + j] = a;
                sr[r] = w32((int64_t)sr[r] + w32((int64_t)cr - hcr[r][idx + j])); si[r] = w32((int64_t)si[r] + w32((int64_t)ci - hci[r][idx + j]));
                hcr[r][idx + j] = cr; hci[r][idx + j] = ci;
                pr[r][j] = sr[r]; pi[r][j] = si[r];
                const int32_t e = w32((int64_t)a.re * a.re + (int64_t)a.im * a.im) >> 5;
                se[r] = w32((int64_t)se[r] + w32((int64_t)e - he[r][idx + j]));
                he[r][idx + j] = e;
                pe[r][j] = se[r];
                if ((int64_t)a.re * a.re + (int64_t)a.im * a.im != w32((int64_t)a.re * a.re + (int64_t)a.im * a.im)) wrapped[j] = 1;
                if (e != 0) silent[j] = 0;
                memmove(last[r], last[r] + 1, 63 * sizeof(c16)); last[r][63] = a;
            }
        idx = (idx + 4) % 32;
        for (int j = 0; j < 4; j++) {
            const int32_t re = w32((int64_t)(pr[0][j] >> 1) + (pr[1][j] >> 1)), im = w32((int64_t)(pi[0][j] >> 1) + (pi[1][j] >> 1));
            acorr[j] = (int64_t)((uint64_t)((int64_t)re * re) + (uint64_t)((int64_t)im * im));
            const int32_t v = w32((int64_t)(pe[0][j] >> 1) + (pe[1][j] >> 1));
            energy[j] = (int64_t)v * v;
        }
        int detected = 0;
        for (int i = 0; i < 4; i++) {
            const int64_t den = (int64_t)((uint64_t)ring[his_index] + 1u);                     /* LLONG_MAX + 1 wraps, as the compiled code does */
            const int64_t eb = (den == -1 && energy[i] == INT64_MIN) ? 0 : energy[i] / (den == 0 ? 1 : den);
            if (ring[his_index] == INT64_MAX) branch[8]++;
            if (wrapped[i]) branch[9]++;
            if (silent[i]) branch[10]++;
            if (!found) {
                sense += 1;
                if (eb > 5 && acorr[i] > (energy[i] >> 1)) { sense = 0; count++; found = 1; }
                else count = 0;
            } else if (acorr[i] < (energy[i] >> 3)) {
                const int good = (int32_t)count > 96 && (int32_t)count < 160;
                found = 0; count = 0;
                if (good) {
                    s[W_READING] = (uint32_t)((uint64_t)ring[his_index] >> 32);
                    s[W_STATE] = 1; detected = 1; branch[i]++;
                    break;                                                                     /* the rest of the burst is neither looked at nor recorded */
                }
                branch[4]++;
            } else {
                count++;
                if ((int32_t)count > 160) { found = 0; count = 0; branch[5]++; }
            }
            ring[his_index++] = energy[i];
            his_index %= 64;
        }
        if (sense >= 84 && !detected) {
            if (flags & FLAG_REARM) { sense = 0; found = 0; count = 0; s[W_TIMEOUTS]++; branch[6]++; }
            else { s[W_ERR] = E_CS_TIMEOUT; branch[7]++; }
        }
    }
    s[W_SENSE] = sense; s[W_FOUND] = (uint32_t)found; s[W_COUNT] = count; s[W_HIS] = his_index;
    for (int k = 0; k < 64; k++) { s[W_RING + 2 * k] = (uint32_t)(uint64_t)ring[k]; s[W_RING + 2 * k + 1] = (uint32_t)((uint64_t)ring[k] >> 32); }
    memcpy(&s[W_HIST], last[0], 256); memcpy(&s[W_HIST + 64], last[1], 256);
    return used;
}

/* ---- T11aDesc: dec[len + 2] -> out[len] */
void st11a_desc(const uint8_t* dec, uint32_t len, uint8_t* out)
{
    uint8_t lut[128];
    for (int i = 0; i < 128; i++) {
        uint8_t x = (uint8_t)(i << 1);
        for (int k = 0; k < 8; k++) { const uint8_t o1 = ((x >> 1) ^ (x >> 4)) & 1; x = (uint8_t)((x >> 1) | (o1 << 7)); }
        lut[i] = x;
    }
    uint8_t reg = (uint8_t)(dec[1] >> 1);
    for (uint32_t i = 0; i < len; i++) { reg = lut[reg]; out[i] = dec[2 + i] ^ reg; reg >>= 1; }
}

/* ---- TBB11aFrameSink over the len bytes of one frame; rec = error_code, frame_crc32 (0, 0 where the brick never decides) */
void st11a_frame_sink(const uint8_t* bytes, uint32_t len, uint32_t* rec)
{
    const uint16_t frame_length = (uint16_t)len;
    uint32_t crc32 = 0xFFFFFFFFu; unsigned long byte_count = 0;
    rec[0] = rec[1] = 0;
    for (uint32_t k = 0; k < frame_length; k++) {
        const uint8_t b = bytes[k];
        if (byte_count < (unsigned long)(frame_length - 4)) {
            byte_count++;
            uint32_t c = (crc32 ^ b) & 0xFFu;
            for (int t = 0; t < 8; t++) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
            crc32 = (crc32 >> 8) ^ c;
        } else if (byte_count < (unsigned long)frame_length) {
            byte_count++;
            if (byte_count == frame_length) {
                uint32_t fcs; memcpy(&fcs, bytes + k - 3, 4);
                rec[1] = fcs;
                rec[0] = ((~crc32) == fcs) ? 0x00000001u : 0x80000006u;
                return;
            }
        }
    }
}
