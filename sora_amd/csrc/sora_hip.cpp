// sora_hip.cpp -- host side of libsora_hip.so: the C ABI of include/sora_hip.h.
//
// Owns, per handle: up to four pipelines (a HIP stream, the look-up tables in HBM and every intermediate array of the
// receive path, sized once from sora_rx_cfg, see rx_types.h) used round-robin by consecutive process calls.  There is NO CPU compute path here:
// every entry point either enqueues HIP kernels or fails.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/sora_hip.h"
#include "kernels.h"
#include "host_trellis.h"
#include "host_stage.h"

using namespace sora;

static thread_local std::string g_last_error;
hipError_t sora_internal_stream_create(hipStream_t* out, int index)
{
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    const int level = index % 3, prio = level == 0 ? 0 : level == 1 ? greatest : least;
    if (least != greatest) return hipStreamCreateWithPriority(out, hipStreamNonBlocking, prio);
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

static int fail(int code, const char* what, hipError_t e = hipSuccess)
{
    char buf[256];
    if (e != hipSuccess) snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof(buf), "%s", what);
    g_last_error = buf;
    return code;
}

// ------------------------------------------------------------------------------------------------
// Look-up tables, regenerated from closed forms (each was checked entry-for-entry against the reference header it
// replaces; the oracle's copies of the same closed forms are sha256-pinned in tests/test_oracle_luts.py, and every GPU
// parity test exercises these).
struct HostTables {
    std::vector<int16_t> usin, ucos, uatan2;
    std::vector<uint8_t> demap;
    std::vector<uint32_t> tw64, tw16, sts, crc, tw128, tw32, tw8, rot;
    std::vector<uint16_t> deint;
    std::vector<uint8_t> scr, scr_seq, scr_phase;
    std::vector<uint32_t> crcz;
    std::vector<uint32_t> trk;           // TrkTables as words
};

static inline uint32_t pk(int re, int im) { return ((uint32_t)re & 0xFFFFu) | ((uint32_t)im << 16); }

// host-side reference IFFT<64> is NOT needed: the STS pattern is the fixed-point IFFT of a constant
// vector, computed once below with the same integer butterflies as the device FFT (conjugate form).
namespace hostfft {
struct c { int re, im; };
static inline int w16(int v) { return (int)(short)v; }
static inline int sat(int v) { return v > 32767 ? 32767 : (v < -32768 ? -32768 : v); }
static inline c mk(int r, int i) { c x; x.re = r; x.im = i; return x; }
static inline c sra(c a, int n) { return mk(a.re >> n, a.im >> n); }
static inline c adds(c a, c b) { return mk(sat(a.re + b.re), sat(a.im + b.im)); }
static inline c subs(c a, c b) { return mk(sat(a.re - b.re), sat(a.im - b.im)); }
static inline c cnot(c a) { return mk(~a.re, ~a.im); }
static inline c conj_mul_shift15(c a, c b)      // a*conj(b)>>15 (vector128.h:1215-1231)
{
    int v0 = (int)((unsigned)(a.re * b.re) + (unsigned)(a.im * b.im));
    int v1 = (int)((unsigned)(a.im * b.re) + (unsigned)(w16(-a.re) * b.im));
    return mk(w16(v0 >> 15), w16(v1 >> 15));
}
static void stage(c* x, int n, const std::vector<c>* tw)     // IFFTSSE<N> (ifft_r4dif.h:11-47)
{
    const int q = n / 4;
    for (int e = 0; e < q; e++) {
        c a = sra(x[e], 2), b = sra(x[e + q], 2), cc = sra(x[e + 2 * q], 2), d = sra(x[e + 3 * q], 2);
        c ac = adds(a, cc), bd = adds(b, d), a_c = subs(a, cc), b_d = subs(b, d);
        c jb = mk(~b_d.im, b_d.re);
        x[e] = adds(ac, bd);
        x[e + q] = conj_mul_shift15(subs(ac, bd), tw[1][e]);
        x[e + 2 * q] = conj_mul_shift15(adds(a_c, jb), tw[0][e]);
        x[e + 3 * q] = conj_mul_shift15(subs(a_c, jb), tw[2][e]);
    }
}
static void t4(c* x)                                          // IFFTSSEEx<4> (ifft_r4dif.h:60-83)
{
    c s0 = sra(x[0], 2), s1 = sra(x[1], 2), s2 = sra(x[2], 2), s3 = sra(x[3], 2);
    c A0 = adds(s0, s2), A1 = adds(s1, s3), B0 = adds(cnot(s2), s0), B1 = adds(cnot(s3), s1);
    c B1r = mk(~B1.im, B1.re);
    x[0] = adds(A0, A1); x[1] = adds(cnot(A1), A0); x[2] = adds(B0, B1r); x[3] = adds(cnot(B1r), B0);
}
}  // namespace hostfft

static void build_tables(HostTables& H)
{
    const double GEN_PI = 3.141593;                      // the constant the reference's table generator used
    H.usin.resize(65536); H.ucos.resize(65536); H.uatan2.resize(65536);
    for (int i = 0; i < 65536; i++) {                    // core/inc/intalglut.h:4,3648
        double x = (double)i * GEN_PI / 32768.0;
        H.usin[i] = (int16_t)std::floor(32767.0 * std::sin(x) + 0.5);
        H.ucos[i] = (int16_t)std::floor(32767.0 * std::cos(x) + 0.5);
    }
    H.rot.resize(65536);
    for (int i = 0; i < 65536; i++) H.rot[i] = pk(H.ucos[i], -(int)H.usin[i]);
    for (int yi = 0; yi < 256; yi++)                     // core/inc/intalglut.h:7332
        for (int xi = 0; xi < 256; xi++) {
            int t = (int)(std::atan2((double)(int8_t)yi, (double)(int8_t)xi) * 32768.0 / GEN_PI);
            H.uatan2[yi * 256 + xi] = (int16_t)(t > 32767 ? 32767 : t);
        }
    // DemapperCore step functions (Brick11/src/demapper.h:55-130): {first input value, soft value}
    struct St { int at, val; };
    static const St bpsk[] = {{-128,0},{-30,1},{-17,2},{-8,3},{0,4},{9,5},{18,6},{31,7}};
    static const St q16[]  = {{-128,0},{-70,1},{-67,2},{-65,3},{-63,4},{-61,5},{-58,6},{-55,7},{56,6},{59,5},{62,4},{64,3},{66,2},{68,1},{71,0}};
    static const St q64a[] = {{-128,0},{-68,1},{-65,2},{-63,3},{-61,4},{-60,5},{-58,6},{-55,7},{56,6},{59,5},{61,4},{62,3},{64,2},{66,1},{69,0}};
    static const St q64b[] = {{-128,0},{-98,1},{-96,2},{-94,3},{-92,4},{-90,5},{-89,6},{-86,7},{-37,6},{-34,5},{-32,4},{-30,3},{-29,2},{-27,1},{-24,0},
                              {25,1},{28,2},{30,3},{31,4},{33,5},{35,6},{38,7},{87,6},{90,5},{91,4},{93,3},{95,2},{97,1},{99,0}};
    H.demap.assign(1024, 0);
    auto gen = [&](int w, const St* st, int n) {
        for (int v = -128; v < 128; v++) { int val = 0; for (int k = 0; k < n; k++) if (v >= st[k].at) val = st[k].val; H.demap[w * 256 + (uint8_t)v] = (uint8_t)val; }
    };
    gen(0, bpsk, 8); gen(1, q16, 15); gen(2, q64a, 15); gen(3, q64b, 29);
    // twiddles (core/inc/fft_lut_twiddle.h): trunc(32767 cos), trunc(-32767 sin)
    const double PI = 3.14159265358979323846;
    std::vector<hostfft::c> t64[3], t16[3];
    H.tw64.resize(48); H.tw16.resize(12);
    for (int k = 1; k <= 3; k++) {
        for (int j = 0; j < 16; j++) { double a = 2 * PI * k * j / 64.0; int re = (int)(32767.0 * std::cos(a)), im = (int)(-32767.0 * std::sin(a));
            H.tw64[(k - 1) * 16 + j] = pk(re, im); t64[k - 1].push_back(hostfft::mk(re, im)); }
        for (int j = 0; j < 4; j++)  { double a = 2 * PI * k * j / 16.0; int re = (int)(32767.0 * std::cos(a)), im = (int)(-32767.0 * std::sin(a));
            H.tw16[(k - 1) * 4 + j] = pk(re, im);  t16[k - 1].push_back(hostfft::mk(re, im)); }
    }
    H.tw128.resize(96); H.tw32.resize(24); H.tw8.resize(4);
    for (int k = 1; k <= 3; k++) {
        for (int j = 0; j < 32; j++) { double a = 2 * PI * k * j / 128.0; H.tw128[(k - 1) * 32 + j] = pk((int)(32767.0 * std::cos(a)), (int)(-32767.0 * std::sin(a))); }
        for (int j = 0; j < 8; j++)  { double a = 2 * PI * k * j / 32.0;  H.tw32[(k - 1) * 8 + j]   = pk((int)(32767.0 * std::cos(a)), (int)(-32767.0 * std::sin(a))); }
    }
    H.tw8[0] = pk(32767, 0); H.tw8[1] = pk((int)(32767.0 * std::cos(PI / 4)), (int)(-32767.0 * std::sin(PI / 4)));
    H.tw8[2] = pk(32767, 0); H.tw8[3] = pk((int)(32767.0 * std::cos(3 * PI / 4)), (int)(-32767.0 * std::sin(3 * PI / 4)));
    // STS correlation patterns: Generate80211aSTS<64> (brick/inc/sequence.h:5-33) + cca.hpp:268-277
    {
        hostfft::c f[64]; for (auto& v : f) v = hostfft::mk(0, 0);
        const int M = 10000;
        auto set = [&](int i, int s) { f[i] = hostfft::mk(s * M, s * M); };
        set(4, -1); set(8, -1); set(12, 1); set(16, 1); set(20, 1); set(24, 1);
        set(64 - 24, 1); set(64 - 20, -1); set(64 - 16, 1); set(64 - 12, -1); set(64 - 8, -1); set(64 - 4, 1);
        hostfft::stage(f, 64, t64);
        for (int k = 0; k < 4; k++) hostfft::stage(f + 16 * k, 16, t16);
        for (int k = 0; k < 16; k++) hostfft::t4(f + 4 * k);
        hostfft::c t[64];
        for (int i = 0; i < 64; i++) { int r = 0; for (int b = 0; b < 6; b++) r |= ((i >> b) & 1) << (5 - b); t[i] = f[r]; }
        H.sts.resize(256);
        for (int p = 0; p < 16; p++) for (int i = 0; i < 16; i++) H.sts[p * 16 + i] = pk(t[p + i].re, t[p + i].im);
    }
    // de-interleaver (Brick11/src/deinterleaver.hpp = inverse of interleave.hpp:43-47): out[k] = in[j(k)]
    H.deint.assign(4 * 288, 0);
    const int nbs[4] = {1, 2, 4, 6};
    for (int d = 0; d < 4; d++) {
        const int nb = nbs[d], N = 48 * nb, s = nb / 2 > 1 ? nb / 2 : 1;
        for (int k = 0; k < N; k++) { int i = (N / 16) * (k % 16) + k / 16; int j = s * (i / s) + (i + N - (16 * i) / N) % s; H.deint[d * 288 + k] = (uint16_t)j; }
    }
    H.crc.resize(256);
    for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1; H.crc[i] = c; }
    // parallel CRC (k_finish): Z_m(x) = register x after m zero bytes is linear in x, so it is the xor of 8 nibble look-ups;
    // levels m = 40 * 2^k combine the 64 lanes' 40-byte segment CRCs in a tree
    H.crcz.resize(6 * 8 * 16);
    for (int k = 0; k < 6; k++)
        for (int j = 0; j < 8; j++)
            for (uint32_t v = 0; v < 16; v++) {
                uint32_t c = v << (4 * j);
                for (int z = 0; z < (40 << k); z++) c = (c >> 8) ^ H.crc[c & 0xFF];
                H.crcz[(k * 8 + j) * 16 + v] = c;
            }
    H.scr.resize(128);
    for (int i = 0; i < 128; i++) { uint8_t x = (uint8_t)(i << 1); for (int k = 0; k < 8; k++) { uint8_t o1 = ((x >> 1) ^ (x >> 4)) & 1;
        x = (uint8_t)((x >> 1) | (o1 << 7)); } H.scr[i] = x; }
    // The descrambler (scramble.hpp:319-349) walks reg -> scr[reg] -> reg>>1 ...: a period-127 cycle of 7-bit
    // states.  Lay the cycle out once: position q holds state st[q]; byte produced from that state = scr[st[q]];
    // 8 positions later comes the state of the next byte.
    {
        std::vector<uint8_t> st(127), z(127 + 16);
        // bit sequence z: start from state 1 (bits z[-7..-1] = state bits 0..6)
        uint8_t state = 1;
        std::vector<int> pos_of(128, -1);
        for (int q = 0; q < 127; q++) {
            st[q] = state; pos_of[state] = q;
            // advance ONE bit: new bit = z[n-7]^z[n-4] = state bit0 ^ state bit3; state = (state >> 1) | (bit << 6)
            uint8_t nb = ((state >> 0) ^ (state >> 3)) & 1;
            state = (uint8_t)((state >> 1) | (nb << 6));
        }
        H.scr_seq.resize(127); H.scr_phase.assign(128, 255);
        for (int q = 0; q < 127; q++) H.scr_seq[q] = H.scr[st[q]];
        for (int s7 = 1; s7 < 128; s7++) H.scr_phase[s7] = (uint8_t)pos_of[s7];
    }
    // the tracker's tables folded for LDS (dev_arith.h: TrkTables)
    {
        static_assert(sizeof(TrkTables) % 16 == 0, "TrkTables is copied 16 bytes at a time");
        H.trk.assign(sizeof(TrkTables) / 4, 0u);
        TrkTables& t = *reinterpret_cast<TrkTables*>(H.trk.data());
        for (int i = 0; i <= 16384; i++) t.q[i] = H.usin[i];
        // (the corrections start at zero: trk_usin / trk_ucos return the mirrored quarter wave)
        for (unsigned a = 0; a < 65536; a++) {
            const int ds = H.usin[a] - trk_usin(t, a), dc = H.ucos[a] - trk_ucos(t, a);
            t.e2s[a >> 4] |= ((uint32_t)ds & 3u) << (2u * (a & 15u));            // (a difference beyond +-1 does not fit: trk_tables_exact fails the load)
            t.e2c[a >> 4] |= ((uint32_t)dc & 3u) << (2u * (a & 15u));
        }
        for (int y = 0; y < 128; y++) for (int x = 0; x < 256; x++) t.h[y * 256 + x] = H.uatan2[y * 256 + x];
        for (int x = 0; x < 256; x++) t.h[128 * 256 + x] = (int16_t)-H.uatan2[128 * 256 + x];
    }
}

// every entry of usin / ucos / uatan2 out of the folded tables: the proof that k_track_lds reads what the other kernels read
static bool trk_tables_exact(const HostTables& H)
{
    const TrkTables& t = *reinterpret_cast<const TrkTables*>(H.trk.data());
    for (unsigned a = 0; a < 65536; a++) if (trk_usin(t, a) != H.usin[a] || trk_ucos(t, a) != H.ucos[a]) return false;
    for (int y = -128; y < 128; y++) for (int x = 0; x < 256; x++) if (trk_uatan2_entry(t, y, x) != H.uatan2[(y & 0xFF) * 256 + x]) return false;
    return true;
}

// ------------------------------------------------------------------------------------------------
// The tables are PINNED: they are generated with this host's libm, and a libm that rounds one sine differently -- or a build with
// -ffast-math -- would change decoded bits without any test in this library noticing.  Every table's sha256 is a constant below (taken from a build whose
// tables were compared entry for entry with the reference headers: core/inc/intalglut.h:4,3648,7332, fft_lut_twiddle.h:61433-61600, Brick11/src/demapper.h:55-130,
// dsp_math.h:215-245); the first use of the tables in a process computes the digests and refuses to go on if one differs.
namespace {
struct Sha256 {
    uint32_t h[8] = { 0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u };
    uint8_t buf[64]; size_t nbuf = 0; uint64_t total = 0;
    static uint32_t ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    void block(const uint8_t* p)
    {
        static const uint32_t K[64] = {
            0x428a2f98,0x71374491,0xb5c0fbcf,0xe9b5dba5,0x3956c25b,0x59f111f1,0x923f82a4,0xab1c5ed5,0xd807aa98,0x12835b01,0x243185be,0x550c7dc3,0x72be5d74,0x80deb1fe,0x9bdc06a7,0xc19bf174,
            0xe49b69c1,0xefbe4786,0x0fc19dc6,0x240ca1cc,0x2de92c6f,0x4a7484aa,0x5cb0a9dc,0x76f988da,0x983e5152,0xa831c66d,0xb00327c8,0xbf597fc7,0xc6e00bf3,0xd5a79147,0x06ca6351,0x14292967,
            0x27b70a85,0x2e1b2138,0x4d2c6dfc,0x53380d13,0x650a7354,0x766a0abb,0x81c2c92e,0x92722c85,0xa2bfe8a1,0xa81a664b,0xc24b8b70,0xc76c51a3,0xd192e819,0xd6990624,0xf40e3585,0x106aa070,
            0x19a4c116,0x1e376c08,0x2748774c,0x34b0bcb5,0x391c0cb3,0x4ed8aa4a,0x5b9cca4f,0x682e6ff3,0x748f82ee,0x78a5636f,0x84c87814,0x8cc70208,0x90befffa,0xa4506ceb,0xbef9a3f7,0xc67178f2 };
        uint32_t w[64];
        for (int i = 0; i < 16; i++) w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
        for (int i = 16; i < 64; i++) { const uint32_t s0 = ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = ror(w[i - 2], 17) ^ ror(w[i - 2],
                19) ^ (w[i - 2] >> 10); w[i] = w[i - 16] + s0 + w[i - 7] + s1; }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; i++) {
            const uint32_t t1 = hh + (ror(e, 6) ^ ror(e, 11) ^ ror(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const uint32_t t2 = (ror(a, 2) ^ ror(a, 13) ^ ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    void update(const void* data, size_t n)
    {
        const uint8_t* p = (const uint8_t*)data; total += n;
        while (n) { const size_t k = std::min(n, 64 - nbuf); memcpy(buf + nbuf, p, k); nbuf += k; p += k; n -= k; if (nbuf == 64) { block(buf); nbuf = 0; } }
    }
    std::string hex()
    {
        const uint64_t bits = total * 8; const uint8_t one = 0x80, zero = 0;
        update(&one, 1); while (nbuf != 56) update(&zero, 1);
        uint8_t len[8]; for (int i = 0; i < 8; i++) len[i] = (uint8_t)(bits >> (56 - 8 * i));
        update(len, 8);
        char out[65]; for (int i = 0; i < 8; i++) snprintf(out + 8 * i, 9, "%08x", h[i]);
        return std::string(out, 64);
    }
};
struct TablePin { const char* name; const char* sha256; };
const TablePin kTablePins[] = {
    { "usin", "303884f4e7d2b574a47cfb1aa610b99aa0722bdd0303db2ebf5f27b0c4eea9b6" },
    { "ucos", "92eca3a66ce9f1035e4b84374dd64f991c69da693e8124613505e953a84e184b" },
    { "rot", "0266a6ff7410a9c4720c60965a2e28ca2f4ef2e17df46f89a9e16a27330fd523" },
    { "uatan2", "7a6b394236967f6f6d0ad97e8cb14edb0ab4f6f50df17f54264f6f2abb3a6aeb" },
    { "demap", "1028dd6bbe87a4ac8190f3bdb9628785714b7cb5f649c170574138c059675d99" },
    { "tw64", "b9a69426c357baf5a4338bfd398e5b754922f997044a2b295ed6dc70068bd7bd" },
    { "tw16", "fe8575adcefa7254bc7a07d5f9000b6c0f69d37f042a6b865fcf9c482ebf0ca9" },
    { "sts", "45f304e6f7f2553d44618ef4b6c4afebc914c22e3a334ace20ef35c384ff7ce7" },
    { "deint", "0178a68770023711d77bd5c4b897579856f846ca086f8a9efa8ffac20ba408a4" },
    { "crc", "12f3e0576d447eb37b36d82ba0c1c5481b8f0d12fdc70347ce4a076b229d4c86" },
    { "scr", "79b208c989740a73350771cd9db10902810c4b6b75cb4fd2578bc7adc6162507" },
    { "scr_seq", "76f691c12b4e3d25b4e0606aa540677f02e5c31b3666188853e624e89bbe7452" },
    { "scr_phase", "4945a6c487c65e6fcb57a858d925a69e3fb382dd397099a6e510a4a6f76e0177" },
    { "tw128", "91cc9a797bfd3c35a1c0ce8d972452419000b0b1dab70cdd56b435f5d01ad834" },
    { "tw32", "2a00eb47f9337b725bd5cfe52b6e7a6c696b141f4d4f10fe770fc403d7b3d703" },
    { "tw8", "e54d5a6817c1f2a559297821786fc9d2e58aa55dc2699d64d289e26bea16e348" },
    { "trk", "3be082dbd671d4ac431fd688fa67f4967ae1b48f48612595e68701e30e83a30e" },
    { "crcz", "035d5a8379b2b38f05c16cb38107a51e153fd87dc45d71909ef8c25db84897e7" },
    { "dsp_sincos", "a85b7311f9347b68cb30ddf481a5670b78339f985ec327a1c6d4325dedf9800c" },
    { "dsp_atan", "7b576ae30701be7ab527c540af4d02e23e5b1ae1cc97e3ee83ab6cd63aa6343d" },
};
}  // namespace

static std::string table_digest(const void* data, size_t bytes) { Sha256 s; s.update(data, bytes); return s.hex(); }

// SORA_OK when `name` is a pinned table and the bytes are the pinned ones; SORA_ERR_FAILED otherwise (message in sora_hip_last_error)
int sora_internal_pin_table(const char* name, const void* data, size_t bytes)
{
    const std::string got = table_digest(data, bytes);
    for (const TablePin& t : kTablePins) if (!strcmp(t.name, name)) {
        if (got == t.sha256) return SORA_OK;
        char msg[256];
        snprintf(msg, sizeof msg, "look-up table '%s' does not have its pinned sha256 (this host's libm or the build's floating-point flags generate different tables): got %s",
                 name, got.c_str());
        return fail(SORA_ERR_FAILED, msg);
    }
    return fail(SORA_ERR_FAILED, "look-up table without a pinned digest");
}

template <typename V> static int pin(const char* name, const V& v) { return sora_internal_pin_table(name, v.data(), v.size() * sizeof(v[0])); }
static int pin_host_tables(const HostTables& H)
{
    int rc;
    if ((rc = pin("usin", H.usin)) || (rc = pin("ucos", H.ucos)) || (rc = pin("rot", H.rot)) || (rc = pin("uatan2", H.uatan2)) || (rc = pin("demap", H.demap)) ||
        (rc = pin("tw64", H.tw64)) || (rc = pin("tw16", H.tw16)) || (rc = pin("sts", H.sts)) || (rc = pin("deint", H.deint)) || (rc = pin("crc", H.crc)) ||
        (rc = pin("scr", H.scr)) || (rc = pin("scr_seq", H.scr_seq)) || (rc = pin("scr_phase", H.scr_phase)) || (rc = pin("tw128", H.tw128)) || (rc = pin("tw32", H.tw32)) ||
        (rc = pin("tw8", H.tw8)) || (rc = pin("crcz", H.crcz)) || (rc = pin("trk", H.trk))) return rc;
    if (!trk_tables_exact(H)) return fail(SORA_ERR_FAILED, "the tracker's folded tables (TrkTables) do not reproduce usin / ucos / uatan2");
    return SORA_OK;
}

struct DevTables {
    Tables T{};
    std::vector<void*> allocs;
    int device = -1;
    int8_t* tx_preamble = nullptr;      // 640 COMPLEX8 samples at 40 MHz, then 704 at 44 MHz (k_tx_preamble), built on first use of the transmitter
    uint32_t* tx11n_preamble = nullptr; // [2][1120] COMPLEX16 (tx11n_preamble_host), built on first use of the 802.11n transmitter
    uint32_t* tx_ht40_preamble = nullptr; // [2][1120] COMPLEX16 (k_tx_ht40_preamble), built on first use of the 40 MHz HT transmitter
};

template <typename V>
static int upload(DevTables& D, const V& v, const void** out)
{
    void* p = nullptr;
    const size_t bytes = v.size() * sizeof(v[0]);
    HIPCHK(hipMalloc(&p, bytes));
    D.allocs.push_back(p);
    HIPCHK(hipMemcpy(p, v.data(), bytes, hipMemcpyHostToDevice));
    *out = p;
    return SORA_OK;
}

static int make_dev_tables(DevTables& D)
{
    HostTables H; build_tables(H);
    int rc;
    {
        static std::mutex m; static int pinned = -1;                             // once per process: the tables are a function of the build and the host's libm
        std::lock_guard<std::mutex> lock(m);
        if (pinned < 0) pinned = pin_host_tables(H);
        if (pinned != SORA_OK) return pin_host_tables(H);                        // (again: the message belongs to this thread)
    }
    if ((rc = upload(D, H.usin, (const void**)&D.T.usin))) return rc;
    if ((rc = upload(D, H.ucos, (const void**)&D.T.ucos))) return rc;
    if ((rc = upload(D, H.rot, (const void**)&D.T.rot))) return rc;
    if ((rc = upload(D, H.uatan2, (const void**)&D.T.uatan2))) return rc;
    if ((rc = upload(D, H.demap, (const void**)&D.T.demap))) return rc;
    if ((rc = upload(D, H.tw64, (const void**)&D.T.tw64))) return rc;
    if ((rc = upload(D, H.tw16, (const void**)&D.T.tw16))) return rc;
    if ((rc = upload(D, H.sts, (const void**)&D.T.sts))) return rc;
    if ((rc = upload(D, H.deint, (const void**)&D.T.deint))) return rc;
    if ((rc = upload(D, H.crc, (const void**)&D.T.crc))) return rc;
    if ((rc = upload(D, H.scr, (const void**)&D.T.scr))) return rc;
    if ((rc = upload(D, H.scr_seq, (const void**)&D.T.scr_seq))) return rc;
    if ((rc = upload(D, H.scr_phase, (const void**)&D.T.scr_phase))) return rc;
    if ((rc = upload(D, H.tw128, (const void**)&D.T.tw128))) return rc;
    if ((rc = upload(D, H.tw32, (const void**)&D.T.tw32))) return rc;
    if ((rc = upload(D, H.tw8, (const void**)&D.T.tw8))) return rc;
    if ((rc = upload(D, H.crcz, (const void**)&D.T.crcz))) return rc;
    if ((rc = upload(D, H.trk, (const void**)&D.T.trk))) return rc;
    return SORA_OK;
}
static void free_dev_tables(DevTables& D) { for (void* p : D.allocs) (void)hipFree(p); D.allocs.clear(); }

// per-device tables for the stand-alone stage entry points: created once per device, under a lock (stage calls on
// different handles / threads are independent, include/sora_hip.h)
static std::mutex g_stage_mutex;
static DevTables* device_tables()
{
    static DevTables* tabs[64] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(g_stage_mutex);
    if (!tabs[dev]) {
        DevTables* D = new DevTables();
        if (make_dev_tables(*D) != SORA_OK) { free_dev_tables(*D); delete D; return nullptr; }
        D->device = dev; tabs[dev] = D;
    }
    return tabs[dev];
}

int sora_internal_fail(int code, const char* what, int hip_error) { return fail(code, what, (hipError_t)hip_error); }
int sora_internal_tables(int device, sora::Tables* out)
{
    if (hipSetDevice(device) != hipSuccess) return SORA_ERR_HARDWARE_FAILED;
    DevTables* D = device_tables();
    if (!D) return SORA_ERR_HARDWARE_FAILED;
    *out = D->T; return SORA_OK;
}
const uint32_t* sora_internal_crc_table(int device)
{
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    DevTables* D = device_tables();
    return D ? D->T.crc : nullptr;
}

// ------------------------------------------------------------------------------------------------
// One receive pipeline: a stream, the device arrays of one call in flight, and that call's bookkeeping (its ticket and completion state: host_calls.h).
struct RxPipe : Call {
    sora_rx_cfg cfg{};
    DevTables tabs;
    uint32_t str = 1;
    // capacities
    uint32_t cap_slots = 0, cap_rows = 0;
    // device arrays
    CapDesc* d_caps = nullptr; FrameRow* d_frames = nullptr; FrameCtx* d_fctx = nullptr; uint32_t* d_nframes = nullptr;
    uint8_t* d_soft = nullptr; VitJob* d_jobs = nullptr;        // split decode path only (allocated on its first use)
    // ... the three symbol kernels' tables: slot owners, equalised bins (256 B per slot), rotation parameters
    uint32_t* d_slot_row = nullptr; uint32_t* d_eq = nullptr; TrackRec* d_track = nullptr; uint32_t* d_pil = nullptr;
    // symbol chain: 1 = k_frame (one wave per frame), 3 = k_sym_front -> k_track_lds -> k_sym_back (few frames in flight),
    // 4 = k_pipe: those three AND the window-parallel trellis as one launch (a handful of frames; needs the windowed trellis)
    int  front = 1;
    uint32_t* d_pflags = nullptr; uint32_t pflag_words = 0;     // ... k_pipe's hand-off words (kernels.h PipeArgs), zeroed for every call
    // sora_rx_bind_mpdu: this call's MPDUs go straight to the host's array (last_bound: what the last enqueue / recorded graph carries)
    uint8_t* bound_mpdu = nullptr; size_t bound_bytes = 0; const void* last_bound = nullptr;
    uint32_t pipe_wait_ticks = 2000000; uint32_t* d_note = nullptr;   // ... the bound of its waits (100 MHz ticks) and the handle's host-mapped note "a wait gave up" (sora_rx)
    bool pipe64 = false;                                        // ... its trellis role in the 64-lane form (two units per wave: the handle's calls in flight are few enough for that many workgroups)
    // A call needs its job counters zero, k_pipe's words zero and (three-kernel chain) no symbol slot owned: the call BEFORE it on this pipeline arranges that inside its k_scan
    // (the pipeline's calls alternate between two sets of counters, words 0-3 and 8-11 of the 64-byte block in front of the frame table) -- no fill kernel in front of a call
    // unless counters_ready says that nothing has: the first call, a call recorded into a hipGraph (its arguments are frozen: it always uses set 0 behind its own fill)
    uint32_t parity = 0; bool counters_ready = false;
    // trellis kernel of the split path (host_trellis.h), and the window-parallel one's scratch (on its first use)
    Trellis trellis = Trellis::Lanes64;
    WinScratch win;
    // sora_rx_set_ordered: this call's trellis kernel starts behind the previous call's (wait_for = that call's ev_trellis), so that calls in flight COMPLETE in the order they were
    // submitted -- the front kernels (latency chains) of a call still run beside the trellis of the one before it, and its delivery beside the trellis of the one after it
    hipEvent_t ev_trellis = nullptr, wait_for = nullptr; bool ordered = false;
    uint8_t* d_vout = nullptr; uint8_t* d_mpdu = nullptr; uint32_t* d_njobs = nullptr; uint32_t* d_joblist = nullptr;
    sora_complex16* d_iq_own = nullptr; size_t iq_own_samples = 0;
    uint8_t* d_dump = nullptr; size_t dump_cap = 0;             // sora_rx_process_dump: the raw dump bytes of this pipeline's call
    uint32_t* cont = nullptr; uint32_t* consumed = nullptr;     // stream mode: the HANDLE's continuation records / resume points (not owned by the pipeline)
    sora_frame_result* d_rows = nullptr; uint32_t* d_nrows = nullptr;
    // last call.  Descriptors go up through a pinned staging buffer (a pageable source would make the "async" copy wait for
    // the stream to drain and expose every launch latency of the call) and only when they differ from the resident set.
    std::vector<CapDesc> h_caps;
    CapDesc* h_caps_pinned = nullptr; size_t caps_resident = 0; hipEvent_t ev_caps = nullptr;
    uint32_t ncaps = 0, total_slots = 0;
    bool have_results = false;
    // Opt-in (SORA_HIP_GRAPH=1): a call that repeats the previous one's geometry (same IQ buffer, same capture set) replays
    // the kernel chain as one hipGraph launch.  Off by default: on this path the GPU time per call dwarfs the six enqueues,
    // and instantiating the graph on the second identical call costs more than it saves for short runs.
    bool use_graph = false;
    const void* last_iq = nullptr; bool last_valid = false;
    hipGraph_t graph = nullptr; hipGraphExec_t graph_exec = nullptr;
    // profiling
    bool profiling = false;
    hipEvent_t ev[9] = {};
    bool ev_valid = false;       // ev[] hold a call whose durations have not been folded into t_sum yet
    double t_sum[8] = {}; uint64_t t_calls = 0;   // per-kernel durations (ms) summed over the profiled calls of this pipeline
    // tool hook (sora_internal_rx_timeline): when set, every profiled call also leaves its kernel boundaries as ms since *tl_base
    std::vector<float>* tl = nullptr; hipEvent_t* tl_base = nullptr; int index = 0;
    unsigned extra = 0;          // tool hook (sora_internal_rx_extra): empty kernel launches appended to every call's chain (what does a packet cost?)
    unsigned only = 0xF;         // tool hook (sora_internal_rx_only): which kernels of the chain a call launches (1 scan, 2 frame, 4 trellis, 8 finish)
};

// Probe hooks (which kernels of the chain a call launches, empty launches appended to a call, the calls' kernel boundaries on one time base, the device arrays between the
// kernels) exist in the TOOLS variant of the library only -- sora_amd.build.build_variant("tools", ["SORA_TOOLS"]), loaded by the scripts under tools/ through SORA_HIP_LIB.
// The product build has neither the entry points nor the branches they steer.
#ifdef SORA_TOOLS
#define RX_ONLY(rx, bit) (((rx)->only & (bit)) != 0u)
#define SORA_TOOL_HOOK __attribute__((visibility("default")))
#else
#define RX_ONLY(rx, bit) true
#endif
static constexpr size_t kNumTimed = 5;
static const char* const kKernelNames[kNumTimed] = { "memset+caps", "k_scan", "k_frame", "k_viterbi", "k_finish" };
// (sora_rx_kernel_name_fused: the removed k_decode chain, kept in the ABI; "" = not launched)
static const char* const kKernelNamesFused[kNumTimed] = { "memset+caps", "k_scan", "k_decode", "", "k_finish" };

namespace sora {
// n16 16-byte words <- 0, then m16 of `ones` <- all ones,
__global__ void __launch_bounds__(256) k_clear16(uint4* __restrict__ p, uint32_t n16, uint4* __restrict__ ones = nullptr, uint32_t m16 = 0,
                                                 // then k16 of `z2` <- 0
                                                 uint4* __restrict__ z2 = nullptr, uint32_t k16 = 0)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
    else if (i - n16 < m16) ones[i - n16] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    else if (i - n16 - m16 < k16) z2[i - n16 - m16] = make_uint4(0u, 0u, 0u, 0u);
}
}  // namespace sora

// Adds the durations of the pipeline's last profiled call to its running sums (waits for that call).
static int fold_profile(RxPipe* rx)
{
    if (!rx->ev_valid) return SORA_OK;
    HIPCHK(hipEventSynchronize(rx->ev[kNumTimed]));
    for (size_t i = 0; i < kNumTimed; i++) { float t = 0.f; HIPCHK(hipEventElapsedTime(&t, rx->ev[i], rx->ev[i + 1])); rx->t_sum[i] += t; }
#ifdef SORA_TOOLS
    if (rx->tl && rx->tl_base && *rx->tl_base && rx->tl->size() < (size_t)(1u << 22)) {
        rx->tl->push_back((float)rx->index);
        for (size_t i = 0; i <= kNumTimed; i++) { float t = 0.f; HIPCHK(hipEventElapsedTime(&t, *rx->tl_base, rx->ev[i])); rx->tl->push_back(t); }
    }
#endif
    rx->t_calls++; rx->ev_valid = false;
    return SORA_OK;
}

static void rx_free(RxPipe* rx)
{
    if (!rx) return;
    void* ptrs[] = { rx->d_caps, rx->d_fctx, rx->d_nframes,
                     rx->d_soft, rx->d_jobs, rx->d_vout, rx->d_mpdu, rx->d_iq_own, rx->d_rows, rx->d_nrows, rx->d_njobs, rx->d_joblist, rx->d_dump, rx->d_slot_row, rx->d_eq, rx->d_track, rx->d_pil,
                     rx->d_pflags };
    for (void* p : ptrs) if (p) (void)hipFree(p);
    rx->win.free();
    for (auto& e : rx->ev) if (e) (void)hipEventDestroy(e);
    if (rx->ev_trellis) (void)hipEventDestroy(rx->ev_trellis);
    if (rx->graph_exec) (void)hipGraphExecDestroy(rx->graph_exec);
    if (rx->graph) (void)hipGraphDestroy(rx->graph);
    if (rx->ev_caps) (void)hipEventDestroy(rx->ev_caps);
    if (rx->ev_done) (void)hipEventDestroy(rx->ev_done);
    if (rx->h_caps_pinned) (void)hipHostFree(rx->h_caps_pinned);
    free_dev_tables(rx->tabs);
    if (rx->stream) (void)hipStreamDestroy(rx->stream);
    delete rx;
}

extern "C" {

int sora_hip_abi_version(void) { return SORA_HIP_ABI_VERSION; }
const char* sora_hip_last_error(void) { return g_last_error.c_str(); }

int sora_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
// ---- the pinned look-up tables, by name (include/sora_hip.h)
namespace { struct NamedTable { const char* name; const void* host; size_t bytes; const void* const* dev; }; }
static std::vector<NamedTable> named_tables(const HostTables& H, const std::vector<uint32_t>& sc, const std::vector<short>& at, const Tables* T,
        const uint32_t* const* dsc, const short* const* dat)
{
#define NT(n, v, d) { n, (v).data(), (v).size() * sizeof((v)[0]), (const void* const*)(d) }
    return { NT("usin", H.usin, T ? &T->usin : nullptr), NT("ucos", H.ucos, T ? &T->ucos : nullptr), NT("rot", H.rot, T ? &T->rot : nullptr), NT("uatan2",
            H.uatan2, T ? &T->uatan2 : nullptr),
             NT("demap", H.demap, T ? &T->demap : nullptr), NT("tw64", H.tw64, T ? &T->tw64 : nullptr), NT("tw16", H.tw16, T ? &T->tw16 : nullptr), NT("sts",
                     H.sts, T ? &T->sts : nullptr),
             NT("deint", H.deint, T ? &T->deint : nullptr), NT("crc", H.crc, T ? &T->crc : nullptr), NT("scr", H.scr, T ? &T->scr : nullptr), NT("scr_seq",
                     H.scr_seq, T ? &T->scr_seq : nullptr),
             NT("scr_phase", H.scr_phase, T ? &T->scr_phase : nullptr), NT("tw128", H.tw128, T ? &T->tw128 : nullptr), NT("tw32", H.tw32,
                     T ? &T->tw32 : nullptr), NT("tw8", H.tw8, T ? &T->tw8 : nullptr),
             NT("crcz", H.crcz, T ? &T->crcz : nullptr), NT("trk", H.trk, T ? &T->trk : nullptr), NT("dsp_sincos", sc, dsc), NT("dsp_atan", at, dat) };
#undef NT
}
int sora_hip_table_count(void) { return (int)(sizeof(kTablePins) / sizeof(kTablePins[0])); }
const char* sora_hip_table_name(int index) { return index >= 0 && index < sora_hip_table_count() ? kTablePins[index].name : nullptr; }
const char* sora_hip_table_pin(const char* name) { for (const TablePin& t : kTablePins) if (name && !strcmp(t.name, name)) return t.sha256; return nullptr; }
// the digest of table `name` as THIS build on THIS host generates it (no device needed): what make_dev_tables compares with the pin
int sora_hip_table_digest(const char* name, char hex65[65])
{
    if (!name || !hex65) return fail(SORA_ERR_INVALID_PARAM, "sora_hip_table_digest: null argument");
    HostTables H; build_tables(H);
    std::vector<uint32_t> sc; std::vector<short> at; sora_internal_dsp_host_tables(sc, at);
    if (!strcmp(name, "trk") && !trk_tables_exact(H)) return fail(SORA_ERR_FAILED, "the tracker's folded tables (TrkTables) do not reproduce usin / ucos / uatan2");
    for (const NamedTable& t : named_tables(H, sc, at, nullptr, nullptr, nullptr)) if (!strcmp(t.name, name)) {
        const std::string d = table_digest(t.host, t.bytes);
        memcpy(hex65, d.c_str(), 65);
        return SORA_OK;
    }
    return fail(SORA_ERR_INVALID_PARAM, "sora_hip_table_digest: no such table");
}
// the DEVICE-RESIDENT copy of table `name` on the current device (the stage entry points' tables; a handle's own copies come from the same generator), read back
int sora_hip_table_read(const char* name, void* h_out, size_t cap, size_t* bytes)
{
    if (!name || !bytes) return fail(SORA_ERR_INVALID_PARAM, "sora_hip_table_read: null argument");
    DevTables* D = device_tables();
    if (!D) return fail(SORA_ERR_HARDWARE_FAILED, "sora_hip_table_read: no tables on this device");
    const uint32_t* dsc = nullptr; const short* dat = nullptr;
    if (!strncmp(name, "dsp_", 4) && sora_internal_dsp_tables(&dsc, &dat) != SORA_OK) return fail(SORA_ERR_HARDWARE_FAILED, "sora_hip_table_read: dsp_math tables");
    HostTables H; build_tables(H);
    std::vector<uint32_t> sc; std::vector<short> at; sora_internal_dsp_host_tables(sc, at);
    for (const NamedTable& t : named_tables(H, sc, at, &D->T, &dsc, &dat)) if (!strcmp(t.name, name)) {
        *bytes = t.bytes;
        if (!h_out) return SORA_OK;
        if (cap < t.bytes) return fail(SORA_ERR_CAPACITY, "sora_hip_table_read: buffer too small");
        HIPCHK(hipMemcpy(h_out, *t.dev, t.bytes, hipMemcpyDeviceToHost));
        return SORA_OK;
    }
    return fail(SORA_ERR_INVALID_PARAM, "sora_hip_table_read: no such table");
}

void* sora_hip_malloc(size_t bytes) { void* p = nullptr; if (hipMalloc(&p, bytes) != hipSuccess) return nullptr; return p; }
void  sora_hip_free(void* p) { if (p) (void)hipFree(p); }
int   sora_hip_memcpy_h2d(void* d, const void* h, size_t n) { HIPCHK(hipMemcpy(d, h, n, hipMemcpyHostToDevice)); return SORA_OK; }
int   sora_hip_stream_synchronize(void* stream) { HIPCHK(hipStreamSynchronize((hipStream_t)stream)); return SORA_OK; }
int   sora_hip_memcpy_d2h(void* h, const void* d, size_t n) { HIPCHK(hipMemcpy(h, d, n, hipMemcpyDeviceToHost)); return SORA_OK; }
int   sora_hip_memcpy_d2d(void* dd, const void* ds, size_t n, void* stream) { HIPCHK(hipMemcpyAsync(dd, ds, n, hipMemcpyDeviceToDevice, (hipStream_t)stream)); return SORA_OK; }
void* sora_hip_host_alloc(size_t bytes) { void* p = nullptr; if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr; return p; }
void  sora_hip_host_free(void* p) { if (p) (void)hipHostFree(p); }

static int pipe_create(const sora_rx_cfg* cfg, RxPipe** out, int index = 0)
{
    if (!cfg || !out || cfg->struct_size != sizeof(sora_rx_cfg)) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_create: bad cfg");
    if (cfg->sample_rate_mhz != 20 && cfg->sample_rate_mhz != 40 && cfg->sample_rate_mhz != 44) return fail(SORA_ERR_INVALID_PARAM, "sample_rate_mhz must be 20, 40 or 44");
    if (cfg->max_captures == 0 || cfg->max_total_samples == 0 || cfg->max_frames_per_capture == 0) return fail(SORA_ERR_INVALID_PARAM, "zero capacity");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SORA_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(SORA_ERR_INVALID_PARAM, "device ordinal out of range");
    HIPCHK(hipSetDevice(cfg->device));
    RxPipe* rx = new RxPipe();
    rx->cfg = *cfg;
    if (rx->cfg.cca_pwr_threshold == 0) rx->cfg.cca_pwr_threshold = 1000 * 1000;
    rx->str = cfg->sample_rate_mhz == 20 ? 1 : 2;
    rx->tabs.device = cfg->device;
    int rc = make_dev_tables(rx->tabs);
    if (rc) { rx_free(rx); return rc; }
    // The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues PER PRIORITY LEVEL (default 4, one of the normal
    // level's is the null stream's): eight pipelines of one priority run three at a time (profiles/r03_e_timeline_*.txt).  Spreading the
    // handle's pipelines over the three levels gives every one of them a hardware queue of its own WITHOUT the application having to set an
    // environment variable before HIP starts.  The levels only order dispatch among kernels that are ready at the same
    // moment; every pipeline's chain is sequential, so none of them starves (profiles/r04_m_stream_priorities.txt).
    hipError_t e = sora_internal_stream_create(&rx->stream, index);
    if (e != hipSuccess) { rx_free(rx); return fail(SORA_ERR_HARDWARE_FAILED, "hipStreamCreate", e); }
    e = hipHostMalloc((void**)&rx->h_caps_pinned, sizeof(CapDesc) * cfg->max_captures, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&rx->ev_caps, hipEventDisableTiming);
    if (e != hipSuccess) { rx_free(rx); return fail(SORA_ERR_HARDWARE_FAILED, "pinned descriptor buffer", e); }
    const uint64_t n20 = cfg->max_total_samples / rx->str;
    // Symbol slots, frame rows and the byte offsets derived from them are 32-bit on the device: a configuration that would
    // wrap them is refused here instead of decoding garbage later.
    const uint64_t want_slots = n20 / 80 + cfg->max_captures + 16, want_rows = (uint64_t)cfg->max_captures * cfg->max_frames_per_capture;
    if (want_slots * (1ull * kSoftBytesPerSlot) + kSoftPad >= (1ull << 32) || want_rows >= (1ull << 31) / 3 || cfg->max_total_samples >= (1ull << 32)) {
        rx_free(rx);
        return fail(SORA_ERR_CAPACITY, "sora_rx_create: max_total_samples / max_captures x max_frames_per_capture exceed the 32-bit slot geometry of one handle "
                                       "(split the batch over several handles)");
    }
    rx->cap_slots = (uint32_t)want_slots;
    rx->cap_rows = (uint32_t)want_rows;
    struct { void** p; size_t bytes; } allocs[] = {
        { (void**)&rx->d_caps, sizeof(CapDesc) * cfg->max_captures },
        { (void**)&rx->d_fctx, sizeof(FrameCtx) * ((size_t)rx->cap_rows + cfg->max_captures) }, { (void**)&rx->d_nframes, 4 * (size_t)cfg->max_captures },
        { (void**)&rx->d_vout, (size_t)kOutPerSlot * rx->cap_slots }, { (void**)&rx->d_mpdu, (size_t)kOutPerSlot * rx->cap_slots },
        { (void**)&rx->d_rows, sizeof(sora_frame_result) * rx->cap_rows },
        { (void**)&rx->d_nrows, 4 }, { (void**)&rx->d_joblist, 3 * 4 * (size_t)rx->cap_rows },
        // the three job counters AND, 64 bytes on, the frame table: one fill clears both at the start of a call
        { (void**)&rx->d_njobs, 64 + sizeof(FrameRow) * rx->cap_rows },
    };
    for (auto& a : allocs) {
        e = hipMalloc(a.p, a.bytes);
        if (e != hipSuccess) { rx_free(rx); return fail(SORA_ERR_HARDWARE_FAILED, "hipMalloc (receive-path arrays)", e); }
    }
    rx->d_frames = reinterpret_cast<FrameRow*>(reinterpret_cast<uint8_t*>(rx->d_njobs) + 64);
    *out = rx;
    return SORA_OK;
}

static void pipe_destroy(RxPipe* rx) { if (rx) { (void)hipSetDevice(rx->cfg.device); (void)hipStreamSynchronize(rx->stream); rx_free(rx); } }

static int pipe_reset(RxPipe* rx)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    HIPCHK(hipSetDevice(rx->cfg.device));
    HIPCHK(hipStreamSynchronize(rx->stream));
    rx->ncaps = 0; rx->total_slots = 0; rx->have_results = false; rx->h_caps.clear(); rx->ticket = 0; rx->delivered = rx->released = false;
    return SORA_OK;
}

static int pipe_flush(RxPipe* rx)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    HIPCHK(hipSetDevice(rx->cfg.device));
    HIPCHK(hipStreamSynchronize(rx->stream));
    return SORA_OK;
}

static void* pipe_stream(RxPipe* rx) { return rx ? (void*)rx->stream : nullptr; }

static int pipe_process_dev(RxPipe* rx, const sora_complex16* d_iq, const sora_capture_desc* caps, size_t ncaps, uint64_t iq_samples = 0)
{
    if (!rx || (!d_iq && ncaps) || (!caps && ncaps)) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_process_dev: null argument");
    if (ncaps > rx->cfg.max_captures) return fail(SORA_ERR_CAPACITY, "more captures than sora_rx_cfg.max_captures");
    HIPCHK(hipSetDevice(rx->cfg.device));
    std::vector<CapDesc> hc(ncaps);                                              // validated first: a refused call leaves the handle's last call intact
    uint64_t total = 0, slots64 = 0;
    for (size_t i = 0; i < ncaps; i++) {
        if (caps[i].offset & 3) return fail(SORA_ERR_INVALID_PARAM, "capture offset must be a multiple of 4 samples (16-byte alignment, memsource.hpp:59)");
        CapDesc& c = hc[i];
        c.offset = caps[i].offset; c.nsamples = caps[i].nsamples; c.capture_id = caps[i].capture_id;
        c.slot_base = (uint32_t)slots64; c.nslots = (caps[i].nsamples / rx->str) / 80 + 1;
        slots64 += c.nslots; total += caps[i].nsamples;
        if (iq_samples && (caps[i].offset > iq_samples || caps[i].nsamples > iq_samples - caps[i].offset))
            return fail(SORA_ERR_INVALID_PARAM, "a capture descriptor reaches past the end of the sample buffer");
    }
    if (total > rx->cfg.max_total_samples || slots64 > rx->cap_slots) return fail(SORA_ERR_CAPACITY, "more samples than sora_rx_cfg.max_total_samples");
    if (rx->bound_mpdu && rx->bound_bytes < (size_t)kOutPerSlot * slots64) {
        rx->bound_mpdu = nullptr;
        return fail(SORA_ERR_CAPACITY, "sora_rx_bind_mpdu: the bound array is smaller than the call's sora_rx_mpdu_bytes()");
    }
    const uint32_t slots = (uint32_t)slots64;
    rx->h_caps.swap(hc);
    rx->ncaps = (uint32_t)ncaps; rx->total_slots = slots; rx->have_results = false; rx->delivered = rx->released = false;
    if (ncaps == 0) { rx->have_results = true; return SORA_OK; }
    if (!rx->d_soft) {                                                           // the soft streams and the job table, on the first call
        // one pre-scaled byte per soft value and the pad behind the last slot (rx_types.h).  Zeroed once: every byte a trellis lane can fetch, written yet or not, is
        // a well-formed value
        const size_t soft_bytes = (size_t)kSoftBytesPerSlot * rx->cap_slots + kSoftPad;
        HIPCHK(hipMalloc((void**)&rx->d_soft, soft_bytes));
        HIPCHK(hipMemsetAsync(rx->d_soft, 0, soft_bytes, rx->stream));
        HIPCHK(hipMalloc((void**)&rx->d_jobs, 3 * sizeof(VitJob) * rx->cap_rows));
    }
    const bool windowed = rx->trellis == Trellis::Windowed;
    // the window-parallel trellis's arrays, on its first use (... and the count of calls whose data field k_win_redo_finish_pipe made again)
    if (windowed) { const int rc = rx->win.ensure(rx->cap_rows, nullptr, true); if (rc) return rc; }
    const bool split = rx->front >= 3;
    // (the handle only asks for k_pipe where its workgroups are all resident at once: pipe_fits)
    const bool pipe = split && rx->front == 4 && windowed;
    if (pipe && !rx->d_pflags) {
        rx->pflag_words = (4u + 4u * rx->cap_rows + (rx->cap_slots + 63u) / 64u + 4u + 3u) / 4u * 4u;
        HIPCHK(hipMalloc((void**)&rx->d_pflags, 4 * ((size_t)rx->pflag_words + 1024)));   // (+ the tools variant's time stamps)
    }
    // the three-kernel symbol chain's arrays, on its first use: slot owners, equalised bins (256 B per slot), pilots, rotation parameters
    if (split && !rx->d_slot_row) {
        HIPCHK(hipMalloc((void**)&rx->d_slot_row, 4 * ((size_t)rx->cap_slots + 64)));
        HIPCHK(hipMalloc((void**)&rx->d_eq, 256 * ((size_t)rx->cap_slots + 64)));
        HIPCHK(hipMalloc((void**)&rx->d_track, sizeof(TrackRec) * ((size_t)rx->cap_slots + 64)));
        HIPCHK(hipMalloc((void**)&rx->d_pil, 16 * ((size_t)rx->cap_slots + 64)));
    }
    hipStream_t st = rx->stream;
    const bool prof = rx->profiling;
    if (prof) { const int rc = fold_profile(rx); if (rc) return rc; }
    int evi = 0;
    auto mark = [&]() { if (prof) (void)hipEventRecord(rx->ev[evi++], st); };
    mark();
    bool caps_changed = false;
    if (rx->caps_resident != ncaps || memcmp(rx->h_caps_pinned, rx->h_caps.data(), sizeof(CapDesc) * ncaps) != 0) {
        if (rx->caps_resident) HIPCHK(hipEventSynchronize(rx->ev_caps));        // the staging buffer's last upload has left it
        memcpy(rx->h_caps_pinned, rx->h_caps.data(), sizeof(CapDesc) * ncaps);
        HIPCHK(hipMemcpyAsync(rx->d_caps, rx->h_caps_pinned, sizeof(CapDesc) * ncaps, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(rx->ev_caps, st));
        rx->caps_resident = ncaps;
        caps_changed = true;
    }
    const uint32_t nrows = rx->ncaps * rx->cfg.max_frames_per_capture;

    auto enqueue = [&](bool recording) -> int {                                  // the kernel chain of one call, in stream order (recording: into a hipGraph)
#ifdef SORA_TOOLS
        // (the tools variant's partial chains and array dumps want the plain protocol: a fill in front of every call)
        const bool self_clean = false;
#else
        const bool self_clean = !recording;
#endif
        const bool fill = !self_clean || !rx->counters_ready;
        const uint32_t par = fill ? 0u : rx->parity;
        uint32_t* const counters = rx->d_njobs + 8u * par;
        const uint32_t pipe_words = pipe ? 4u + 4u * nrows + (slots + 63u) / 64u : 0u;
        if (fill && RX_ONLY(rx, 1u)) {
            // the job counters and the frame table behind them, the slot owners (no symbol slot has an owner yet; only the three-kernel chain reads them) and k_pipe's hand-off
            // words: ONE fill (every packet of a call costs the command processor a few microseconds: DESIGN.md section 3.6) -- by a kernel of this library: a hipMemsetAsync
            // of 64 + 64 n bytes recorded into a hipGraph faults on replay
            // (the owners' array has 64 words of slack)
            const uint32_t n16 = (uint32_t)((64 + sizeof(FrameRow) * (size_t)nrows) / 16), m16 = split ? (slots + 3) / 4 : 0u;
            const uint32_t k16 = (pipe_words + 3u) / 4u;
            hipLaunchKernelGGL(k_clear16, dim3((n16 + m16 + k16 + 255) / 256), dim3(256), 0, st, reinterpret_cast<uint4*>(rx->d_njobs), n16,
                               reinterpret_cast<uint4*>(rx->d_slot_row), m16, reinterpret_cast<uint4*>(rx->d_pflags), k16);
        }
        ScanArgs S{};
        S.iq = reinterpret_cast<const uint32_t*>(d_iq); S.caps = rx->d_caps; S.ncaps = rx->ncaps; S.str = rx->str;
        S.keep_queue = rx->cfg.sample_rate_mhz == 44 ? 1u : 0u; S.thr = rx->cfg.cca_pwr_threshold;
        S.max_frames = rx->cfg.max_frames_per_capture; S.T = rx->tabs.T; S.frames = rx->d_frames; S.fctx = rx->d_fctx; S.nframes = rx->d_nframes;
        S.njobs = counters; S.joblist = rx->d_joblist; S.nrows = nrows; S.slot_row = split ? rx->d_slot_row : nullptr; S.cont = rx->cont; S.consumed = rx->consumed;
        // this call's k_scan prepares the next one's (and its own slot owners and hand-off words)
        if (self_clean) {
            S.zero_a = rx->d_njobs + 8u * (1u - par); S.nzero_a = 4; S.zero_b = pipe ? rx->d_pflags : nullptr; S.nzero_b = pipe_words; S.own_slots = 1;
        }
        rx->parity = self_clean ? 1u - par : 0u; rx->counters_ready = self_clean;
        mark();
        if (RX_ONLY(rx, 1u)) hipLaunchKernelGGL(k_scan, dim3(rx->ncaps), dim3(64), 0, st, S);
        mark();

        RxArgs R{};
        R.iq = S.iq; R.caps = rx->d_caps; R.str = rx->str; R.total_slots = slots; R.nrows = nrows; R.T = rx->tabs.T;
        R.frames = rx->d_frames; R.fctx = rx->d_fctx;
        R.vout = rx->d_vout; R.mpdu = rx->d_mpdu; R.njobs = counters; R.joblist = rx->d_joblist; R.mpdu_host = rx->bound_mpdu;
        R.soft = rx->d_soft; R.jobs = rx->d_jobs; R.slot_row = rx->d_slot_row; R.eq = rx->d_eq; R.track = rx->d_track; R.pil = rx->d_pil;
        R.pipe_flags = pipe ? rx->d_pflags : nullptr;
        // behind the window-parallel trellis the proof, the decode of what fails it and T11aDesc / the frame sink are ONE launch: the wave that holds a pair of frames
        // finishes them
        const bool redo_finish = windowed && RX_ONLY(rx, 4u) && RX_ONLY(rx, 8u);
        // the call's job table: three code-rate lists of nrows jobs behind this call's counters
        const TrellisJobs J = trellis_lists(rx->d_jobs, counters, nrows, nrows);
        const uint32_t pair_groups = trellis_pair_groups(J);

        // the symbol chain
        if (pipe) {
            // a handful of frames: the symbol chain AND the window-parallel trellis as one launch (k_rx.hip: k_pipe), the proof behind it
            if (RX_ONLY(rx, 2u)) {
                PipeArgs P{};
                P.nfront = (slots + 63) / 64; P.ntrack = nrows; P.flags = rx->d_pflags; P.target = kWinUnitsTarget; P.vstride = rx->win.stride;
                P.vecs = rx->win.d_vecs; P.stamp_base = rx->pflag_words;
                P.lanes64 = rx->pipe64 ? 1u : 0u; P.wait_ticks = rx->pipe_wait_ticks;
                // trellis waves: those of k_viterbi16w, or -- 64-lane form -- unit u of two frames each
                const uint32_t waves = rx->pipe64 ? kWinMaxUnits * ((nrows + 3) / 2) : trellis_win_waves(J);
                hipLaunchKernelGGL(k_pipe, dim3(P.nfront + P.ntrack + (waves + 3) / 4), dim3(256), 0, st, R, P);
            }
            mark();
            if (RX_ONLY(rx, 4u) && !redo_finish) trellis_proof<256>(J, rx->d_soft, rx->d_vout, rx->win, st);
        } else if (split) {
            // The symbol chain as three kernels (k_rx.hip): per symbol slot in front of and behind the tracker, per frame (four lanes each) for the tracker, whose tables
            // are in LDS: the chain for FEW frames in flight, where k_frame's one wave per frame is a 465-symbol serial loop (fsample-6).
            if (RX_ONLY(rx, 2u)) {
                hipLaunchKernelGGL(k_sym_front, dim3((slots + 63) / 64), dim3(256), 0, st, R);
                hipLaunchKernelGGL(k_track_lds, dim3((nrows + 63) / 64), dim3(256), 0, st, R);
                hipLaunchKernelGGL(k_sym_back, dim3((slots + 63) / 64), dim3(256), 0, st, R);
            }
        } else if (RX_ONLY(rx, 2u)) hipLaunchKernelGGL(k_frame, dim3((nrows + 3) / 4), dim3(256), 0, st, R);
        mark();

        // the trellis (k_pipe holds it itself)
        if (!pipe) {
            if (rx->wait_for && !recording) (void)hipStreamWaitEvent(st, rx->wait_for, 0);   // (sora_rx_set_ordered: behind the previous call's trellis)
            // (window-parallel: the proof is the finisher's, below, unless the finisher is not launched)
            if (RX_ONLY(rx, 4u)) trellis_launch<256>(rx->trellis, J, rx->d_soft, rx->d_vout, st, rx->win, !redo_finish);
            if (rx->ordered && !recording && rx->ev_trellis) (void)hipEventRecord(rx->ev_trellis, st);
            mark();
        }

        // the finish (behind k_pipe: ... and the plain chain's code for the whole call if a wait inside k_pipe gave up)
        if (redo_finish && pipe)
            hipLaunchKernelGGL(k_win_redo_finish_pipe, dim3(pair_groups), dim3(256), 0, st, J.jobs, J.hdr, nrows, kWinUnitsTarget,
                               rx->win.stride, (const uint16_t*)rx->win.d_vecs, (const uint8_t*)rx->d_soft, rx->d_vout, rx->win.d_stats, R, rx->d_note);
        else if (redo_finish)
            hipLaunchKernelGGL(k_win_redo_finish, dim3(pair_groups), dim3(256), 0, st, J.jobs, J.hdr, nrows, kWinUnitsTarget,
                               rx->win.stride, (const uint16_t*)rx->win.d_vecs, (const uint8_t*)rx->d_soft, rx->d_vout, rx->win.d_stats, R);
        else if (RX_ONLY(rx, 8u)) hipLaunchKernelGGL(k_finish, dim3((nrows + 3) / 4), dim3(256), 0, st, R);
#ifdef SORA_TOOLS
        for (unsigned x = 0; x < rx->extra; x++) hipLaunchKernelGGL(k_clear16, dim3(1), dim3(256), 0, st, reinterpret_cast<uint4*>(rx->d_njobs), 0u);
#endif
        mark();
        return SORA_OK;
    };

    const bool repeat = rx->last_valid && !caps_changed && rx->last_iq == (const void*)d_iq && rx->last_bound == (const void*)rx->bound_mpdu;
    rx->last_bound = rx->bound_mpdu;
    if (!repeat && rx->graph_exec) {
        (void)hipGraphExecDestroy(rx->graph_exec); rx->graph_exec = nullptr;
        (void)hipGraphDestroy(rx->graph); rx->graph = nullptr;
    }
    rx->last_iq = d_iq; rx->last_valid = true;
    bool launched = false;
    if (rx->use_graph && !prof && repeat && !rx->ordered) {                      // (an ordered call waits for an event of another stream: the plain launches)
        if (!rx->graph_exec) {                                                   // second identical call: record the chain
            if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                const int rc = enqueue(true);
                hipGraph_t g = nullptr;
                const hipError_t e2 = hipStreamEndCapture(st, &g);
                if (rc == SORA_OK && e2 == hipSuccess && g && hipGraphInstantiate(&rx->graph_exec, g, nullptr, nullptr, 0) == hipSuccess) rx->graph = g;
                else { if (g) (void)hipGraphDestroy(g); rx->graph_exec = nullptr; rx->use_graph = false; (void)hipGetLastError(); }
            } else { rx->use_graph = false; (void)hipGetLastError(); }
        }
        if (rx->graph_exec) { HIPCHK(hipGraphLaunch(rx->graph_exec, st)); launched = true; }
    }
    if (!launched) { const int rc = enqueue(false); if (rc) return rc; }
    HIPCHK(hipGetLastError());
    rx->ev_valid = prof;
    rx->have_results = true;
    return SORA_OK;
}

static int pipe_process(RxPipe* rx, const sora_complex16* h_iq, size_t total_samples, const sora_capture_desc* caps, size_t ncaps)
{
    if (!rx || !h_iq) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_process: null argument");
    if (total_samples > rx->cfg.max_total_samples) return fail(SORA_ERR_CAPACITY, "more samples than sora_rx_cfg.max_total_samples");
    HIPCHK(hipSetDevice(rx->cfg.device));
    if (rx->iq_own_samples < total_samples) {
        if (rx->d_iq_own) (void)hipFree(rx->d_iq_own);
        rx->d_iq_own = nullptr; rx->iq_own_samples = 0;
        HIPCHK(hipMalloc((void**)&rx->d_iq_own, sizeof(sora_complex16) * (total_samples + 64)));
        rx->iq_own_samples = total_samples;
    }
    HIPCHK(hipMemcpyAsync(rx->d_iq_own, h_iq, sizeof(sora_complex16) * total_samples, hipMemcpyHostToDevice, rx->stream));
    return pipe_process_dev(rx, rx->d_iq_own, caps, ncaps, total_samples);
}

// LoadSoraDumpFile -> graph as ONE stream-ordered path (brickutil.h:20-58 in front of fb11a_demod.cpp:88-120): the dump bytes go up from
// (preferably page-locked) host memory, sora_hip_ingest de-frames / sign-fixes / resamples / decimates them on the device, and the receive
// chain runs on the result -- all on this pipeline's stream, no host wait.  The capture descriptors address the INGESTED stream.
static int pipe_process_dump(RxPipe* rx, const void* h_dump, size_t dump_bytes, unsigned flags, const sora_capture_desc* caps, size_t ncaps)
{
    if (!rx || !h_dump || dump_bytes == 0) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_process_dump: null argument");
    if ((flags & ~15u) || (dump_bytes & 3)) return fail(SORA_ERR_INVALID_PARAM,
            "sora_rx_process_dump: unknown ingest flag, or a dump that is not a whole number of 4-byte samples");
    const size_t n = sora_hip_ingest_count(dump_bytes, flags);
    if (n > rx->cfg.max_total_samples) return fail(SORA_ERR_CAPACITY, "sora_rx_process_dump: the dump holds more samples than sora_rx_cfg.max_total_samples");
    HIPCHK(hipSetDevice(rx->cfg.device));
    // (growing: the previous call of this pipeline may still read them)
    if (rx->dump_cap < dump_bytes || rx->iq_own_samples < n) HIPCHK(hipStreamSynchronize(rx->stream));
    if (rx->dump_cap < dump_bytes) {
        if (rx->d_dump) (void)hipFree(rx->d_dump);
        rx->d_dump = nullptr; rx->dump_cap = 0;
        HIPCHK(hipMalloc((void**)&rx->d_dump, dump_bytes + 256));
        rx->dump_cap = dump_bytes;
    }
    if (rx->iq_own_samples < n) {
        if (rx->d_iq_own) (void)hipFree(rx->d_iq_own);
        rx->d_iq_own = nullptr; rx->iq_own_samples = 0;
        HIPCHK(hipMalloc((void**)&rx->d_iq_own, sizeof(sora_complex16) * (n + 64)));
        rx->iq_own_samples = n;
    }
    HIPCHK(hipMemcpyAsync(rx->d_dump, h_dump, dump_bytes, hipMemcpyHostToDevice, rx->stream));
    size_t got = 0;
    const int rc = sora_hip_ingest(rx->d_dump, dump_bytes, flags, rx->d_iq_own, rx->iq_own_samples, &got, (void*)rx->stream);
    if (rc != SORA_OK) return rc;
    return pipe_process_dev(rx, rx->d_iq_own, caps, ncaps, got);
}

static int pipe_pack(RxPipe* rx)                                                // dense rows of the pipeline's call -> d_rows / d_nrows, in stream order
{
    static_assert(sizeof(sora_frame_result) == 36, "sora_frame_result layout");
    if (rx->ncaps == 0) HIPCHK(hipMemsetAsync(rx->d_nrows, 0, 4, rx->stream));
    else hipLaunchKernelGGL(k_pack, dim3(1), dim3(1024), 0, rx->stream, (const FrameRow*)rx->d_frames, (const uint32_t*)rx->d_nframes,
                            (const CapDesc*)rx->d_caps, rx->ncaps, rx->cfg.max_frames_per_capture, reinterpret_cast<PackedRow*>(rx->d_rows), rx->d_nrows);
    HIPCHK(hipGetLastError());
    return SORA_OK;
}

static int pipe_results(RxPipe* rx, sora_frame_result* out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap)
{
    if (!rx || !nout) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_results: null argument");
    *nout = 0;
    if (!rx->have_results) return fail(SORA_ERR_FAILED, "no process call to report");
    if (rx->ncaps == 0) return SORA_OK;
    HIPCHK(hipSetDevice(rx->cfg.device));
    { const int rc = pipe_pack(rx); if (rc) return rc; }
    uint32_t nrows = 0;
    HIPCHK(hipMemcpyAsync(&nrows, rx->d_nrows, 4, hipMemcpyDeviceToHost, rx->stream));
    HIPCHK(hipStreamSynchronize(rx->stream));
    std::vector<sora_frame_result> rows(nrows);
    if (nrows) HIPCHK(hipMemcpy(rows.data(), rx->d_rows, sizeof(sora_frame_result) * (size_t)nrows, hipMemcpyDeviceToHost));
    std::vector<uint8_t> mp;
    if (h_mpdu && nrows) { mp.resize((size_t)kOutPerSlot * rx->total_slots); HIPCHK(hipMemcpy(mp.data(), rx->d_mpdu, mp.size(), hipMemcpyDeviceToHost)); }
    size_t n = 0, moff = 0; int rc = SORA_OK;
    for (uint32_t i = 0; i < nrows; i++) {
        if (n >= max_out) { rc = SORA_ERR_CAPACITY; break; }
        sora_frame_result& o = out[n++];
        o = rows[i];
        const size_t src = o.mpdu_offset;                                        // slot0 * 32 in the device array
        o.mpdu_offset = (uint32_t)moff;                                          // dense in the caller's buffer
        if (h_mpdu && (o.error_code == E_FRAME_OK || o.error_code == E_CRC32_FAIL)) {
            if (moff + o.length > mpdu_cap) { rc = SORA_ERR_CAPACITY; continue; }
            memcpy(h_mpdu + moff, mp.data() + src, o.length);
            moff += o.length;
        }
    }
    *nout = n;
    if (rc != SORA_OK) return fail(rc, "sora_rx_results: output buffer too small");
    return SORA_OK;
}

static int pipe_set_profiling(RxPipe* rx, int enable)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    HIPCHK(hipSetDevice(rx->cfg.device));
    if (enable && !rx->ev[0]) for (auto& e : rx->ev) HIPCHK(hipEventCreate(&e));
    rx->profiling = enable != 0; rx->ev_valid = false;
    for (auto& t : rx->t_sum) t = 0.0;
    rx->t_calls = 0;
    return SORA_OK;
}

const char* sora_rx_kernel_name(size_t i) { return i < kNumTimed ? kKernelNames[i] : ""; }
const char* sora_rx_kernel_name_fused(size_t i) { return i < kNumTimed ? kKernelNamesFused[i] : ""; }

static int pipe_results_dev(RxPipe* rx, const sora_frame_result** d_rows, const uint32_t** d_nrows, const uint8_t** d_mpdu)
{
    if (!rx) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_results_dev: null handle");
    if (!rx->have_results) return fail(SORA_ERR_FAILED, "no process call to report");
    HIPCHK(hipSetDevice(rx->cfg.device));
    { const int rc = pipe_pack(rx); if (rc) return rc; }
    if (d_rows) *d_rows = rx->d_rows;
    if (d_nrows) *d_nrows = rx->d_nrows;
    if (d_mpdu) *d_mpdu = rx->d_mpdu;
    return SORA_OK;
}

// Result delivery without a host wait: pack, then copy rows / count / MPDU array behind the call's kernels on its own stream.
// (Measured and dropped in round 3: ONE kernel writing the three ranges into the mapped host buffers itself instead of three copies --
// no blit launches, no ~50 us of queue idle time between them -- made the step 19 % slower, 0.53 -> 0.63 ms: waves stalled on PCIe
// writes hold CU slots the other calls' kernels need.  profiles/r03_j_deliver_kernel.txt.)
static int pipe_deliver_async(RxPipe* rx, sora_frame_result* h_rows, size_t max_rows, uint32_t* h_nrows, uint8_t* h_mpdu, size_t mpdu_bytes)
{
    if (!rx || !h_rows || !h_nrows) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_deliver_async: null argument");
    if (!rx->have_results) return fail(SORA_ERR_FAILED, "no process call to report");
    const size_t need = (size_t)kOutPerSlot * rx->total_slots;
    // (checked before anything is enqueued)
    if (h_mpdu && mpdu_bytes < need) return fail(SORA_ERR_CAPACITY, "sora_rx_deliver_async: h_mpdu is smaller than sora_rx_mpdu_bytes()");
    HIPCHK(hipSetDevice(rx->cfg.device));
    { const int rc = pipe_pack(rx); if (rc) return rc; }
    const size_t nr = std::min<size_t>(max_rows, (size_t)rx->ncaps * rx->cfg.max_frames_per_capture);
    HIPCHK(hipMemcpyAsync(h_nrows, rx->d_nrows, 4, hipMemcpyDeviceToHost, rx->stream));
    if (nr) HIPCHK(hipMemcpyAsync(h_rows, rx->d_rows, sizeof(sora_frame_result) * nr, hipMemcpyDeviceToHost, rx->stream));
    // (a call bound to this very array has written its MPDUs there already: sora_rx_bind_mpdu)
    if (h_mpdu && need && h_mpdu != rx->bound_mpdu) HIPCHK(hipMemcpyAsync(h_mpdu, rx->d_mpdu, need, hipMemcpyDeviceToHost, rx->stream));
    HIPCHK(call_mark_delivered(*rx));
    return SORA_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// The public handle: up to kMaxDepth pipelines used round-robin by consecutive process calls, so that the latency-bound
// front end of one call (k_scan) overlaps the issue-bound decode kernel of the call before it -- the overlap
// the reference gets from running ViterbiThread beside RxThread (fb11a_demod.cpp:117-120, TThreadSeparator
// stdbrick.hpp:89-248).  Independent streams with no cross-stream events: kernels of different calls share the CUs.
// captures in flight (depth x the handle's max_captures) from which the automatic choice is k_viterbi16: below that the
// window-parallel form wins (gpurun r05: one to four 4096-capture calls in flight 0.60 / 0.51 / 0.48 / 0.46 ms per call
// against 0.71 / 0.52 / 0.51 / 0.51 for the better of the two serial kernels; eight calls: k_viterbi16 0.40 against 0.42)
constexpr long long kAutoLanes16Captures = 32768;
struct sora_rx {
    static constexpr int kMaxDepth = 16;
    sora_rx_cfg cfg{};
    std::atomic<int> depth{8};   // (read by other handles' automatic kernel choice under g_rx_mu)
    TrellisChoice trellis;       // sora_rx_set_trellis: no value = chosen from the depth
    int front = 0;               // sora_rx_set_front: 0 = chosen from the capacity in flight, 1 = k_frame, 3 = the three-kernel symbol chain
    bool use_graph = false;
    int cur = 0;                 // pipeline of the most recent process call
    bool started = false;
    bool profiling = false;
    int seq = 0;                 // ticket of the most recent process call
    RxPipe* pipes[kMaxDepth] = {};
    StreamRecords records{kContWords};                                            // sora_rx_set_stream_mode
    // tool hook (sora_internal_rx_timeline)
    std::vector<float> tl; hipEvent_t tl_base = nullptr;
    // k_pipe's safety net: the bound of the waits inside its launch; the host-mapped word its finishing kernel sets when one of them gave up (the call's rows are
    // right all the same: k_rx.hip, k_win_redo_finish_pipe); the calls this handle then keeps to the three-kernel chain; how often that happened
    uint32_t pipe_wait_us = 20000;
    uint32_t* h_note = nullptr; uint32_t* d_note = nullptr;
    int pipe_backoff = 0; unsigned long long pipe_backoffs = 0;
    uint8_t* next_bound = nullptr; size_t next_bound_bytes = 0;               // sora_rx_bind_mpdu: for the next process call only
    bool ordered = false; hipEvent_t last_trellis = nullptr;                      // sora_rx_set_ordered
    std::atomic<long long> last_call_ns{0};   // when this handle last took a process call (steady clock): what OTHER handles' automatic kernel choice looks at (chip_is_shared)
};

// The handles of this process, for ONE question: is the chip being kept full by somebody else?  k_pipe is the chain for an otherwise idle chip (each of its workgroups
// takes a whole CU's LDS: beside a full chip its launch waits for CUs to drain, tools/pipe_under_load.py), so a handle's automatic choice leaves it alone while another
// handle of the process on the same device -- one sized for a batch -- has taken a call within the last few milliseconds.  (Other processes are not seen.)
constexpr int kPipeBackoffCalls = 64;       // calls a handle keeps to the three-kernel chain after a wait inside one of its k_pipe launches gave up
static std::mutex g_rx_mu;
static std::vector<sora_rx*> g_rx_all;
static std::atomic<long long> g_shared_window_ns{20000000};     // 20 ms (sora_hip_set_share_window_us: a test -- or a host with its own idea of "recently" -- sets it)
constexpr long long kBatchRows = 1024;                          // frame rows in flight from which a handle counts as one that fills the chip
static long long steady_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static bool chip_is_shared(const sora_rx* me)
{
    const long long now = steady_ns();
    std::lock_guard<std::mutex> lk(g_rx_mu);
    for (const sora_rx* h : g_rx_all) {
        if (h == me || h->cfg.device != me->cfg.device) continue;
        const long long rows = (long long)h->depth * (long long)h->cfg.max_captures * (long long)h->cfg.max_frames_per_capture;
        const long long t = h->last_call_ns.load(std::memory_order_relaxed);
        if (rows >= kBatchRows && t != 0 && now - t < g_shared_window_ns.load(std::memory_order_relaxed)) return true;
    }
    return false;
}

static RxPipe* pipe_at(sora_rx* rx, int i)
{
    if (!rx->pipes[i]) {
        if (pipe_create(&rx->cfg, &rx->pipes[i], i) != SORA_OK) return nullptr;
        rx->pipes[i]->use_graph = rx->use_graph;
        if (rx->profiling) (void)pipe_set_profiling(rx->pipes[i], 1);
        rx->pipes[i]->tl = &rx->tl; rx->pipes[i]->tl_base = &rx->tl_base; rx->pipes[i]->index = i;
        rx->pipes[i]->d_note = rx->d_note;
    }
    return rx->pipes[i];
}

extern "C" {

int sora_rx_create(const sora_rx_cfg* cfg, sora_rx_t** out)
{
    if (!out) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_create: bad cfg");
    RxPipe* p0 = nullptr;
    const int rc = pipe_create(cfg, &p0);
    if (rc != SORA_OK) return rc;
    sora_rx* rx = new sora_rx();
    rx->cfg = *cfg; rx->pipes[0] = p0;
    // (host-mapped, written by k_win_redo_finish_pipe; without it the safety net still works, the handle just does not learn from it)
    if (hipHostMalloc((void**)&rx->h_note, 64, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer((void**)&rx->d_note, rx->h_note, 0) == hipSuccess) *rx->h_note = 0;
    else { (void)hipGetLastError(); if (rx->h_note) (void)hipHostFree(rx->h_note); rx->h_note = rx->d_note = nullptr; }
    p0->d_note = rx->d_note;
    { std::lock_guard<std::mutex> lk(g_rx_mu); g_rx_all.push_back(rx); }
    *out = rx;
    return SORA_OK;
}

void sora_rx_destroy(sora_rx_t* rx)
{
    if (!rx) return;
    { std::lock_guard<std::mutex> lk(g_rx_mu); g_rx_all.erase(std::remove(g_rx_all.begin(), g_rx_all.end(), rx), g_rx_all.end()); }
    for (RxPipe* p : rx->pipes) if (p) pipe_destroy(p);
    rx->records.free();
    if (rx->tl_base) (void)hipEventDestroy(rx->tl_base);
    if (rx->h_note) (void)hipHostFree(rx->h_note);
    delete rx;
}

// k_decode (the data field in one kernel) has been removed: the switch stays in the ABI, always off
int sora_rx_set_fused(sora_rx_t* rx, int enable)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    if (enable > 0) return fail(SORA_E_NOT_SUPPORTED, "sora_rx_set_fused: k_decode has been removed from the library");
    return 0;
}

// Which trellis kernel a call uses: k_viterbi16 pays off once enough frames are in flight to give every SIMD a wave of it (it packs
// eight frames into a wave, k_viterbi two); see DESIGN.md section 3.1.  What counts is the handle's capacity in flight, not the number
// of tickets: two calls of 16384 captures fill the chip like eight of 4096, and eight calls of 64 captures do not.
static Trellis trellis_for(const sora_rx* rx)                                   // -> RxPipe::trellis
{
    if (rx->trellis) return *rx->trellis;
    return (long long)rx->depth * (long long)rx->cfg.max_captures >= kAutoLanes16Captures ? Trellis::Lanes16 : Trellis::Windowed;
}

// The symbol chain: one wave per frame (k_frame) is the cheaper one when the chip is full of frames; the three-kernel chain spreads a frame's symbols over the
// chip and runs the tracker's chain out of LDS: the one for few, long frames.
// frame rows in flight (depth x max_captures x max_frames_per_capture) up to which the automatic choice is the three-kernel chain
constexpr long long kAutoSplitRows = 512;
// ... and up to which it is k_pipe (the chain and the window-parallel trellis as one launch), if that launch fits
constexpr long long kAutoPipeRows = 16;
// k_pipe's workgroups wait for one another inside the launch: it is only used where ALL workgroups of ALL the handle's calls in flight are resident at once -- one per CU
// (160 KB of LDS each), and a good part of the chip left to whatever else runs
static uint64_t device_cus(int device)                                         // compute units of the device (the partition this process sees), looked up once
{
    static std::mutex mu; static std::vector<int> cus;
    std::lock_guard<std::mutex> lk(mu);
    if ((size_t)device >= cus.size()) cus.resize((size_t)device + 1, 0);
    if (cus[device] == 0) { hipDeviceProp_t pr; cus[device] = hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256; }
    return (uint64_t)cus[device];
}
static uint64_t pipe_groups(const sora_rx* rx, bool lanes64)                   // workgroups of one k_pipe launch of this handle
{
    const uint64_t str = rx->cfg.sample_rate_mhz == 20 ? 1 : 2, rows = (uint64_t)rx->cfg.max_captures * rx->cfg.max_frames_per_capture;
    const uint64_t slots = rx->cfg.max_total_samples / str / 80 + rx->cfg.max_captures + 16;
    const uint64_t waves = lanes64 ? (uint64_t)kWinMaxUnits * ((rows + 3) / 2) : win_waves(rows);
    return (slots + 63) / 64 + rows + (waves + 3) / 4;
}
// frame rows in flight up to which the automatic choice is k_pipe
// Is handle h one whose calls are k_pipe launches right now (as far as another handle can tell without asking front_for, which asks this)?
static bool pipe_candidate(const sora_rx* h, long long now)
{
    if (h->front != 4 && h->front != 0) return false;
    if (h->trellis && *h->trellis != Trellis::Windowed) return false;
    const long long rows = (long long)h->depth * (long long)h->cfg.max_captures * (long long)h->cfg.max_frames_per_capture;
    if (h->front == 0 && rows > kAutoPipeRows) return false;
    const long long t = h->last_call_ns.load(std::memory_order_relaxed);
    return t != 0 && now - t < g_shared_window_ns.load(std::memory_order_relaxed);
}
// The CUs are shared by every handle of the process on the device: the launches of ALL of them that are k_pipe's (each workgroup a whole CU's LDS) must be resident together
static bool pipe_fits(const sora_rx* rx, bool lanes64 = false)
{
    const uint64_t rows = (uint64_t)rx->cfg.max_captures * rx->cfg.max_frames_per_capture;
    uint64_t groups = pipe_groups(rx, lanes64) * (uint64_t)rx->depth;
    {
        const long long now = steady_ns();
        std::lock_guard<std::mutex> lk(g_rx_mu);
        for (const sora_rx* h : g_rx_all)
            if (h != rx && h->cfg.device == rx->cfg.device && pipe_candidate(h, now)) groups += pipe_groups(h, false) * (uint64_t)h->depth;
    }
    // (64-lane form: every frame must come out cut into single windows, i.e. get its full 80 units: kWinUnitsTarget / 80 frames at most)
    return groups <= device_cus(rx->cfg.device) * 3 / 4 && (!lanes64 || rows * (uint64_t)rx->depth <= 204);   // (three quarters of the CUs: 192 of an MI355X's 256)
}
static int front_for(const sora_rx* rx)                                        // -> RxPipe::front
{
    if (rx->front == 1 || rx->front == 3) return rx->front;
    // (a wait inside one of this handle's k_pipe launches gave up a few calls ago: somebody else -- another process, other GPU work -- holds CUs; the chain for a while)
    const bool can_pipe = rx->pipe_backoff == 0 && trellis_for(rx) == Trellis::Windowed && pipe_fits(rx);
    if (rx->front == 4) return can_pipe ? 4 : 3;
    const long long rows = (long long)rx->depth * (long long)rx->cfg.max_captures * (long long)rx->cfg.max_frames_per_capture;
    return rows <= kAutoPipeRows && can_pipe && !chip_is_shared(rx) ? 4 : rows <= kAutoSplitRows ? 3 : 1;
}
int sora_rx_set_front(sora_rx_t* rx, int kernels)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    const int old = rx->front;
    if (kernels == 0 || kernels == 1 || kernels == 3 || kernels == 4) {
        rx->front = kernels;
        for (RxPipe* p : rx->pipes) if (p) p->last_valid = false;               // (a recorded hipGraph holds the other kernels)
    } else if (kernels > 0) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_set_front: 0 (automatic), 1 (k_frame), 3 (k_sym_front, k_track_lds, k_sym_back) or 4 (k_pipe)");
    return old;
}
int sora_rx_front(sora_rx_t* rx) { return rx ? front_for(rx) : SORA_ERR_INVALID_PARAM; }
int sora_rx_set_ordered(sora_rx_t* rx, int on)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    const int old = rx->ordered ? 1 : 0;
    if (on == 0 || on == 1) { rx->ordered = on != 0; if (!rx->ordered) rx->last_trellis = nullptr; for (RxPipe* p : rx->pipes) if (p) p->last_valid = false; }
    return old;
}
int sora_rx_call_front(sora_rx_t* rx, int ticket)                              // what call `ticket` WAS launched with: latched at its process call
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    if (ticket == 0) ticket = rx->seq;
    RxPipe* p = call_find(rx->pipes, sora_rx::kMaxDepth, ticket);
    return p ? p->front : fail(SORA_ERR_INVALID_PARAM, "sora_rx_call_front: no call with this ticket is held by the handle");
}
uint32_t sora_hip_set_share_window_us(uint32_t us)
{
    return (uint32_t)(g_shared_window_ns.exchange((long long)us * 1000, std::memory_order_relaxed) / 1000);
}

int sora_rx_set_trellis(sora_rx_t* rx, int lanes_per_pair)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    const int old = trellis_abi(rx->trellis);
    if (trellis_parse(lanes_per_pair, &rx->trellis)) {
        for (RxPipe* p : rx->pipes) if (p) p->last_valid = false;               // (a recorded hipGraph holds the other kernel)
    } else if (lanes_per_pair > 0) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_set_trellis: 0 (automatic), 16 or 64 lanes per frame pair, or SORA_TRELLIS_WINDOWED");
    return old;
}

// boundaries compared, boundaries that differed, frames decoded again by the serial kernel, units -- summed over the handle's pipelines since its creation
int sora_rx_window_stats(sora_rx_t* rx, unsigned long long out[4])
{
    if (!rx || !out) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_window_stats: null argument");
    return win_stats_sum(rx->pipes, sora_rx::kMaxDepth, rx->cfg.device, out);
}

// The NEXT process call's frame sink writes every MPDU straight into the caller's page-locked array as well (same geometry as the device's: sora_frame_result::mpdu_offset of
// sora_rx_deliver_async's rows indexes it); sora_rx_deliver_async with that array then delivers rows and count only.
int sora_rx_bind_mpdu(sora_rx_t* rx, uint8_t* h_mpdu, size_t mpdu_bytes)
{
    if (!rx) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_bind_mpdu: null handle");
    rx->next_bound = h_mpdu; rx->next_bound_bytes = h_mpdu ? mpdu_bytes : 0;
    return SORA_OK;
}

// k_pipe's safety net: the bound of the waits inside its launch ...
int sora_rx_set_pipe_wait_us(sora_rx_t* rx, long long us)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    const int old = (int)rx->pipe_wait_us;
    if (us >= 0) rx->pipe_wait_us = (uint32_t)std::min<long long>(us, 40000000ll);
    return old;
}
// ... and its record: out[0] = calls whose data field the finishing kernel made again because a wait gave up, out[1] = times the handle then left k_pipe alone
int sora_rx_pipe_stats(sora_rx_t* rx, unsigned long long out[2])
{
    if (!rx || !out) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_pipe_stats: null argument");
    HIPCHK(hipSetDevice(rx->cfg.device));
    out[0] = 0;
    for (RxPipe* p : rx->pipes) if (p && p->win.d_stats) {
        unsigned long long v = 0;
        HIPCHK(hipStreamSynchronize(p->stream));
        HIPCHK(hipMemcpy(&v, p->win.redone(), sizeof v, hipMemcpyDeviceToHost));
        out[0] += v;
    }
    if (rx->h_note && *(volatile uint32_t*)rx->h_note != 0u) { *(volatile uint32_t*)rx->h_note = 0u; rx->pipe_backoff = kPipeBackoffCalls; rx->pipe_backoffs++; }
    out[1] = rx->pipe_backoffs;
    return SORA_OK;
}

int sora_internal_rx_device(sora_rx_t* rx) { return rx ? rx->cfg.device : -1; }

int sora_rx_trellis(sora_rx_t* rx) { return rx ? trellis_abi(trellis_for(rx)) : SORA_ERR_INVALID_PARAM; }

int sora_rx_set_graph(sora_rx_t* rx, int enable)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    const int old = rx->use_graph ? 1 : 0;
    if (enable >= 0) { rx->use_graph = enable != 0; for (RxPipe* p : rx->pipes) if (p) { p->use_graph = rx->use_graph; p->last_valid = false; } }
    return old;
}

int sora_rx_set_depth(sora_rx_t* rx, int depth)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    const int old = rx->depth;
    if (depth > 0) rx->depth = std::min(depth, (int)sora_rx::kMaxDepth);
    return old;
}

int sora_rx_reset(sora_rx_t* rx)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    for (RxPipe* p : rx->pipes) if (p) { const int rc = pipe_reset(p); if (rc) return rc; }
    return rx->records.zero(rx->cfg.max_captures);                               // ISource::Reset: every stream starts afresh
}

int sora_rx_flush(sora_rx_t* rx)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    for (RxPipe* p : rx->pipes) if (p) { const int rc = pipe_flush(p); if (rc) return rc; }
    return SORA_OK;
}

void* sora_rx_stream(sora_rx_t* rx) { return rx ? pipe_stream(rx->pipes[rx->cur]) : nullptr; }

// Stream mode: a call continues the one before it, so that one must have finished with the records (its scan) before this one's scan reads
// them -- the calls of a handle in stream mode run one after the other (the host needs the resume points of call n to assemble call n + 1 anyway).
static int stream_prologue(sora_rx* rx, RxPipe* p)
{
    p->cont = nullptr; p->consumed = nullptr;
    if (!rx->records.on) return SORA_OK;
    { const int rc = sora_rx_flush(rx); if (rc) return rc; }
    p->cont = rx->records.d_cont; p->consumed = rx->records.d_consumed; p->last_valid = false;
    return SORA_OK;
}

int sora_rx_set_stream_mode(sora_rx_t* rx, int enable)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    if (enable >= 0) { const int rc = sora_rx_flush(rx); if (rc) return rc; }
    return rx->records.set(enable, rx->cfg.device, rx->cfg.max_captures);
}

int sora_rx_stream_consumed(sora_rx_t* rx, int ticket, uint32_t* h_consumed, size_t ncaps)
{
    if (!rx || !h_consumed) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_stream_consumed: null argument");
    return rx->records.consumed("sora_rx_stream_consumed", rx->cfg.device, call_find(rx->pipes, sora_rx::kMaxDepth, ticket), ticket == rx->seq, h_consumed, ncaps);
}

// Diagnostic (tests): the continuation record k_scan left for one capture of the most recent call (kernels.h: kContWords words; k_scan.hip: cont_store has the layout)
int sora_rx_stream_record_of(sora_rx_t* rx, int ticket, uint32_t capture, uint32_t* h_words, size_t cap_words, size_t* n_words)
{
    if (!rx || !n_words || (!h_words && cap_words)) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_stream_record_of: null argument");
    return rx->records.record_of("sora_rx_stream_record_of", rx->cfg.device, call_find(rx->pipes, sora_rx::kMaxDepth, ticket), ticket == rx->seq, capture, h_words,
                                 cap_words, n_words);
}

// The kernels of the next call on pipeline p (the handle's settings, its capacity in flight, what else the chip is doing).  k_pipe's finishing kernel leaves a note when a
// wait inside that launch gave up (the call's rows are right all the same); the handle then keeps to the three-kernel chain for the next kPipeBackoffCalls calls.
static void choose_kernels(sora_rx* rx, RxPipe* p)
{
    if (rx->h_note && *(volatile uint32_t*)rx->h_note != 0u) { *(volatile uint32_t*)rx->h_note = 0u; rx->pipe_backoff = kPipeBackoffCalls; rx->pipe_backoffs++; }
    else if (rx->pipe_backoff > 0) rx->pipe_backoff--;
    p->bound_mpdu = rx->next_bound; p->bound_bytes = rx->next_bound_bytes; rx->next_bound = nullptr; rx->next_bound_bytes = 0;
    p->ordered = rx->ordered;
    if (p->ordered && !p->ev_trellis && hipEventCreateWithFlags(&p->ev_trellis, hipEventDisableTiming) != hipSuccess) { p->ev_trellis = nullptr; p->ordered = false; (void)hipGetLastError(); }
    p->wait_for = p->ordered && rx->last_trellis != p->ev_trellis ? rx->last_trellis : nullptr;     // (its own previous call is ahead of it in its stream anyway)
    if (p->ordered) rx->last_trellis = p->ev_trellis; else rx->last_trellis = nullptr;
    if (p->trellis != trellis_for(rx)) { p->trellis = trellis_for(rx); p->last_valid = false; }
    { const int fr = front_for(rx); if (p->front != fr) { p->front = fr; p->last_valid = false; } }
    { const bool p64 = p->front == 4 && pipe_fits(rx, true); if (p->pipe64 != p64) { p->pipe64 = p64; p->last_valid = false; } }
    { const uint32_t wt = rx->pipe_wait_us > 40000000u ? 0xFFFFFFFFu : rx->pipe_wait_us * 100u; if (p->pipe_wait_ticks != wt) { p->pipe_wait_ticks = wt; p->last_valid = false; } }
}

int sora_rx_process_dev(sora_rx_t* rx, const sora_complex16* d_iq, const sora_capture_desc* caps, size_t ncaps)
{
    if (!rx) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_process_dev: null argument");
    const int next = call_next(rx->pipes, rx->depth);
    RxPipe* p = pipe_at(rx, next);
    if (!p) return SORA_ERR_HARDWARE_FAILED;
    { const int rc = stream_prologue(rx, p); if (rc) return rc; }
    choose_kernels(rx, p);
    const int rc = pipe_process_dev(p, d_iq, caps, ncaps);
    if (rc == SORA_OK) { rx->cur = next; rx->started = true; p->ticket = ++rx->seq; rx->last_call_ns.store(steady_ns(), std::memory_order_relaxed); }
    return rc;
}

int sora_rx_process(sora_rx_t* rx, const sora_complex16* h_iq, size_t total_samples, const sora_capture_desc* caps, size_t ncaps)
{
    if (!rx) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_process: null argument");
    const int next = call_next(rx->pipes, rx->depth);
    RxPipe* p = pipe_at(rx, next);
    if (!p) return SORA_ERR_HARDWARE_FAILED;
    { const int rc = stream_prologue(rx, p); if (rc) return rc; }
    choose_kernels(rx, p);
    const int rc = pipe_process(p, h_iq, total_samples, caps, ncaps);
    if (rc == SORA_OK) { rx->cur = next; rx->started = true; p->ticket = ++rx->seq; rx->last_call_ns.store(steady_ns(), std::memory_order_relaxed); }
    return rc;
}

int sora_rx_process_dump(sora_rx_t* rx, const void* h_dump, size_t dump_bytes, unsigned ingest_flags, const sora_capture_desc* caps, size_t ncaps)
{
    if (!rx) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_process_dump: null argument");
    const int next = call_next(rx->pipes, rx->depth);
    RxPipe* p = pipe_at(rx, next);
    if (!p) return SORA_ERR_HARDWARE_FAILED;
    { const int rc = stream_prologue(rx, p); if (rc) return rc; }
    choose_kernels(rx, p);
    const int rc = pipe_process_dump(p, h_dump, dump_bytes, ingest_flags, caps, ncaps);
    if (rc == SORA_OK) { rx->cur = next; rx->started = true; p->ticket = ++rx->seq; rx->last_call_ns.store(steady_ns(), std::memory_order_relaxed); }
    return rc;
}

#ifdef SORA_TOOLS
// Test / tool hook (not part of the ABI in include/sora_hip.h): the device arrays between the kernels of the most recent call, for
// stage-by-stage comparisons (tools/dbg_arrays.py).  out[] = { frames, slot_row, eq, track, soft, jobs, joblist, njobs, k_pipe's stamps }; *slots = symbol slots of the call.
SORA_TOOL_HOOK int sora_internal_rx_arrays(sora_rx_t* rx, const void** out, uint32_t* slots, uint32_t* nrows)
{
    if (!rx || !out) return SORA_ERR_INVALID_PARAM;
    RxPipe* p = rx->pipes[rx->cur];
    if (!p) return SORA_ERR_FAILED;
    out[0] = p->d_frames; out[1] = p->d_slot_row; out[2] = p->d_eq; out[3] = p->d_track; out[4] = p->d_soft; out[5] = p->d_jobs; out[6] = p->d_joblist; out[7] = p->d_njobs;
    out[8] = p->d_pflags ? p->d_pflags + p->pflag_words : nullptr;               // k_pipe's time stamps (SORA_DBG_PIPE_TIMELINE)
    if (slots) *slots = p->total_slots;
    if (nrows) *nrows = p->ncaps * p->cfg.max_frames_per_capture;
    return SORA_OK;
}

// Test / tool hook (not part of the ABI in include/sora_hip.h): the next calls launch only the kernels in `mask` (1 k_scan + its memsets, 2 k_frame, 4 the trellis
// kernel, 8 k_finish) and leave the other stages' arrays as the last full call wrote them -- to time one kernel against another (tools/r04_corun.py).
SORA_TOOL_HOOK int sora_internal_rx_only(sora_rx_t* rx, unsigned mask)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    for (int i = 0; i < sora_rx::kMaxDepth; i++) { RxPipe* p = pipe_at(rx, i); if (p) { p->only = mask & 0xFu; p->last_valid = false; } if (i + 1 >= rx->depth) break; }
    return SORA_OK;
}

// Test / tool hook: `n` empty kernel launches behind every call's k_finish (tools/r04_packet_cost.sh).
SORA_TOOL_HOOK int sora_internal_rx_extra(sora_rx_t* rx, unsigned n)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    for (int i = 0; i < rx->depth; i++) { RxPipe* p = pipe_at(rx, i); if (p) { p->extra = n; p->last_valid = false; } }
    return SORA_OK;
}

// Test / tool hook (not part of the ABI in include/sora_hip.h): a timeline of the profiled calls without a profiler attached.  start = 1 records the
// time base (on the first pipeline's stream) and clears the log; every call processed under sora_rx_set_profiling(1) then leaves 1 + 6 floats:
// its pipeline and the boundaries of memset+caps | k_scan | k_frame | trellis | k_finish in ms since the base.  start = 0 copies the log out.
SORA_TOOL_HOOK int sora_internal_rx_timeline(sora_rx_t* rx, int start, float* out, size_t cap, size_t* nout)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    HIPCHK(hipSetDevice(rx->cfg.device));
    if (start) {
        RxPipe* p0 = pipe_at(rx, 0); if (!p0) return SORA_ERR_FAILED;
        if (!rx->tl_base) HIPCHK(hipEventCreate(&rx->tl_base));
        rx->tl.clear();
        for (int i = 0; i < sora_rx::kMaxDepth; i++) if (rx->pipes[i]) { rx->pipes[i]->tl = &rx->tl; rx->pipes[i]->tl_base = &rx->tl_base; rx->pipes[i]->index = i; }
        HIPCHK(hipEventRecord(rx->tl_base, p0->stream));
        HIPCHK(hipEventSynchronize(rx->tl_base));
        return SORA_OK;
    }
    if (!out || !nout) return SORA_ERR_INVALID_PARAM;
    for (RxPipe* p : rx->pipes) if (p) { const int rc = fold_profile(p); if (rc) return rc; }
    *nout = rx->tl.size() < cap ? rx->tl.size() : cap;
    memcpy(out, rx->tl.data(), *nout * sizeof(float));
    return SORA_OK;
}

#endif  // SORA_TOOLS

int sora_rx_results(sora_rx_t* rx, sora_frame_result* out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap)
{
    if (!rx) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_results: null argument");
    return pipe_results(rx->pipes[rx->cur], out, max_out, nout, h_mpdu, mpdu_cap);
}

int sora_rx_results_dev(sora_rx_t* rx, const sora_frame_result** d_rows, const uint32_t** d_nrows, const uint8_t** d_mpdu)
{
    if (!rx) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_results_dev: null handle");
    return pipe_results_dev(rx->pipes[rx->cur], d_rows, d_nrows, d_mpdu);
}

int sora_rx_ticket(sora_rx_t* rx) { return rx && rx->started ? rx->pipes[rx->cur]->ticket : 0; }

// Tickets are looked up, and delivered calls polled, among all kMaxDepth pipelines; the next call is placed among the first `depth`
int sora_rx_wait(sora_rx_t* rx, int ticket)
{
    RxPipe* p = rx ? call_find(rx->pipes, sora_rx::kMaxDepth, ticket) : nullptr;
    return p ? call_wait(p->cfg.device, *p) : call_stale("sora_rx_wait");
}

int sora_rx_wait_any(sora_rx_t* rx, int* ticket)
{
    if (!rx || !ticket) return fail(SORA_ERR_INVALID_PARAM, "sora_rx_wait_any: null argument");
    return calls_wait_any(rx->pipes, sora_rx::kMaxDepth, rx->cfg.device, ticket, "sora_rx", [rx](int t) { return sora_rx_wait(rx, t); });
}

void* sora_rx_stream_of(sora_rx_t* rx, int ticket)
{
    RxPipe* p = rx ? call_find(rx->pipes, sora_rx::kMaxDepth, ticket) : nullptr;
    return p ? pipe_stream(p) : nullptr;
}

int sora_rx_results_of(sora_rx_t* rx, int ticket, sora_frame_result* out, size_t max_out, size_t* nout, uint8_t* h_mpdu, size_t mpdu_cap)
{
    RxPipe* p = rx ? call_find(rx->pipes, sora_rx::kMaxDepth, ticket) : nullptr;
    if (!p) return call_stale("sora_rx_results_of");
    return pipe_results(p, out, max_out, nout, h_mpdu, mpdu_cap);
}

int sora_rx_results_dev_of(sora_rx_t* rx, int ticket, const sora_frame_result** d_rows, const uint32_t** d_nrows, const uint8_t** d_mpdu)
{
    RxPipe* p = rx ? call_find(rx->pipes, sora_rx::kMaxDepth, ticket) : nullptr;
    if (!p) return call_stale("sora_rx_results_dev_of");
    return pipe_results_dev(p, d_rows, d_nrows, d_mpdu);
}

size_t sora_rx_mpdu_bytes(sora_rx_t* rx, int ticket)
{
    RxPipe* p = rx ? call_find(rx->pipes, sora_rx::kMaxDepth, ticket) : nullptr;
    return p ? (size_t)kOutPerSlot * p->total_slots : 0;
}

int sora_rx_deliver_async(sora_rx_t* rx, int ticket, sora_frame_result* h_rows, size_t max_rows, uint32_t* h_nrows, uint8_t* h_mpdu, size_t mpdu_bytes)
{
    RxPipe* p = rx ? call_find(rx->pipes, sora_rx::kMaxDepth, ticket) : nullptr;
    if (!p) return call_stale("sora_rx_deliver_async");
    return pipe_deliver_async(p, h_rows, max_rows, h_nrows, h_mpdu, mpdu_bytes);
}

int sora_rx_set_profiling(sora_rx_t* rx, int enable)
{
    if (!rx) return SORA_ERR_INVALID_PARAM;
    rx->profiling = enable != 0;
    for (RxPipe* p : rx->pipes) if (p) { const int rc = pipe_set_profiling(p, enable); if (rc) return rc; }
    return SORA_OK;
}

int sora_rx_kernel_times(sora_rx_t* rx, float* ms, size_t cap, size_t* nout)
{
    if (!rx || !ms || !nout) return SORA_ERR_INVALID_PARAM;
    *nout = 0;
    double sum[kNumTimed] = {}; uint64_t calls = 0;
    for (RxPipe* p : rx->pipes) if (p) {
        HIPCHK(hipSetDevice(p->cfg.device));
        const int rc = fold_profile(p); if (rc) return rc;
        for (size_t i = 0; i < kNumTimed; i++) sum[i] += p->t_sum[i];
        calls += p->t_calls;
    }
    if (!calls) return fail(SORA_ERR_FAILED, "no profiled process call");
    for (size_t i = 0; i < kNumTimed && i < cap; i++) { ms[i] = (float)(sum[i] / (double)calls); (*nout)++; }
    return SORA_OK;
}

// ---- transmitter (row f2)
static int tx_params(uint32_t kbps, int* nd)
{
    switch (kbps) { case 6000: *nd = 24; return 1; case 9000: *nd = 36; return 1; case 12000: *nd = 48; return 1; case 18000: *nd = 72; return 1;
                    case 24000: *nd = 96; return 1; case 36000: *nd = 144; return 1; case 48000: *nd = 192; return 1; case 54000: *nd = 216; return 1; }
    return 0;
}

size_t sora_hip_tx11a_samples(uint32_t mpdu_len_nofcs, uint32_t rate_kbps)
{
    int nd = 0;
    if (!tx_params(rate_kbps, &nd) || mpdu_len_nofcs + 4 > 4095) return 0;
    const uint32_t ndp = rate_kbps == 9000 ? (uint32_t)nd * 2 : (uint32_t)nd;     // PHY_11a.hpp:120-123
    const uint32_t dbytes = 2 + (mpdu_len_nofcs + 4) + 1;
    const uint32_t rem = (dbytes * 8) % ndp, pad_bits = rem ? ndp - rem : 0;
    const uint32_t nbytes = dbytes + (pad_bits + 7) / 8;
    return 640 + 160 * (size_t)(1 + nbytes * 8 / (uint32_t)nd);
}

// both rates: the 44 MHz form differs in the kernel's last step and in the preamble table alone
static int tx11a_launch(bool up44, const char* who, const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps, const uint8_t* d_seed,
                        size_t nframes, int8_t* d_out, const uint64_t* d_out_off, void* stream)
{
    if (sora_hip_device_count() <= 0) return fail(SORA_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
    if (!d_mpdu || !d_off || !d_len || !d_rate_kbps || !d_seed || !d_out || !d_out_off) return fail(SORA_ERR_INVALID_PARAM, who);
    if (nframes == 0) return SORA_OK;
    DevTables* D = device_tables(); if (!D) return fail(SORA_ERR_HARDWARE_FAILED, "table upload failed");
    hipStream_t st = (hipStream_t)stream;
    {
        // built once per device, under the lock, and complete before it is published: a call on another stream or thread
        // must never see a half-written preamble (640 samples at 40 MHz, then 704 at 44 MHz)
        std::lock_guard<std::mutex> lock(g_stage_mutex);
        if (!D->tx_preamble) {
            int8_t* p = nullptr;
            HIPCHK(hipMalloc((void**)&p, 1280 + 1408));
            hipLaunchKernelGGL(k_tx_preamble, dim3(1), dim3(64), 0, st, p, p + 1280, D->T);
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { (void)hipFree(p); return fail(SORA_ERR_HARDWARE_FAILED, "k_tx_preamble", e); }
            D->tx_preamble = p; D->allocs.push_back(p);
        }
    }
    TxArgs A{};
    A.mpdu = d_mpdu; A.off = d_off; A.len = d_len; A.rate = d_rate_kbps; A.seed = d_seed; A.out8 = d_out; A.out_off = d_out_off;
    A.preamble = D->tx_preamble + (up44 ? 1280 : 0); A.T = D->T;
    if (up44) hipLaunchKernelGGL(k_tx11a<true>, dim3((unsigned)nframes), dim3(256), 0, st, A);
    else      hipLaunchKernelGGL(k_tx11a<false>, dim3((unsigned)nframes), dim3(256), 0, st, A);
    HIPCHK(hipGetLastError());
    return SORA_OK;
}

int sora_hip_tx11a(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps, const uint8_t* d_seed,
                   size_t nframes, int8_t* d_out, const uint64_t* d_out_off, void* stream)
{
    return tx11a_launch(false, "sora_hip_tx11a: null pointer", d_mpdu, d_off, d_len, d_rate_kbps, d_seed, nframes, d_out, d_out_off, stream);
}

size_t sora_hip_tx11a44_samples(uint32_t mpdu_len_nofcs, uint32_t rate_kbps)
{
    return sora_hip_tx11a_samples(mpdu_len_nofcs, rate_kbps) / 10 * 11;          // whole 160-sample blocks, 176 samples each
}

int sora_hip_tx11a44(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps, const uint8_t* d_seed,
                     size_t nframes, int8_t* d_out, const uint64_t* d_out_off, void* stream)
{
    return tx11a_launch(true, "sora_hip_tx11a44: null pointer", d_mpdu, d_off, d_len, d_rate_kbps, d_seed, nframes, d_out, d_out_off, stream);
}

// ---- 802.11n 2x2 transmitter
// The fixed fields of LSrc / HTSrc (preamble11n.hpp:8-83), per chain: L-STF (320), L-LTF (320), HT-STF, HT-LTF1, HT-LTF2 (160 each).
// Each is round(s * sum_k X_k exp(+2 pi i k n / 128)) in double precision -- the standard's frequency-domain sequence X in bins -26..26
// (-28..28 for the HT-LTF) of a 128-point grid, no 1/128 -- repeated or cyclically extended, chain 1 delayed circularly by 8 samples
// (L fields) or 16 (HT fields), HT-LTF2 negated on chain 0 (the 2x2 P matrix).  The scales are fitted to the reference modulator's
// output (tests/golden/refgraph_11n.npz, the first 640 and the 480 from sample 1120 on, both chains, all four frames) and reproduce
// it exactly inside these intervals:
//   L-STF, HT-STF: s = 256 sqrt(2) = 362.039 (exact for s in [361.982, 362.095])
//   L-LTF: s = K / sqrt(52), HT-LTF: s = K / sqrt(56), K = 1773.7209 (exact for K in [1773.7204, 1773.7213], both LTFs together)
static void tx11n_preamble_host(std::vector<uint32_t>& tab)
{
    static const int kLtf[53] = { 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 0,
                                  1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1 };
    static const int kStf[13] = { 1, -1, 1, -1, -1, 1, 0, -1, -1, 1, 1, 1, 1 };        // x (1 + j) on carriers -24, -20, .., 24
    const double K = 1773.7209, pi = 3.14159265358979323846;
    std::vector<double> Xr(128 * 3, 0.0), Xi(128 * 3, 0.0);                                // 0: STF, 1: L-LTF, 2: HT-LTF
    for (int i = 0; i < 13; i++) { const int b = (4 * i - 24) & 127; Xr[b] = kStf[i]; Xi[b] = kStf[i]; }
    for (int i = 0; i < 53; i++) Xr[128 + ((i - 26) & 127)] = kLtf[i];
    for (int i = 0; i < 57; i++) Xr[256 + ((i - 28) & 127)] = i < 2 ? 1 : i > 54 ? -1 : kLtf[i - 2];
    const double scale[3] = { 256.0 * std::sqrt(2.0), K / std::sqrt(52.0), K / std::sqrt(56.0) };
    int16_t t[3][128][2];
    for (int f = 0; f < 3; f++)
        for (int n = 0; n < 128; n++) {
            double re = 0, im = 0;
            for (int k = 0; k < 128; k++) {
                if (Xr[128 * f + k] == 0 && Xi[128 * f + k] == 0) continue;
                const double c = std::cos(2 * pi * k * n / 128), sn = std::sin(2 * pi * k * n / 128);
                re += Xr[128 * f + k] * c - Xi[128 * f + k] * sn; im += Xr[128 * f + k] * sn + Xi[128 * f + k] * c;
            }
            t[f][n][0] = (int16_t)std::llround(scale[f] * re); t[f][n][1] = (int16_t)std::llround(scale[f] * im);
        }
    auto word = [&](int f, int n, int sign) { return (uint32_t)(uint16_t)(sign * t[f][n & 127][0]) | ((uint32_t)(uint16_t)(sign * t[f][n & 127][1]) << 16); };
    tab.assign(2 * kTx11nPreamble, 0);
    for (int ch = 0; ch < 2; ch++) {
        uint32_t* o = tab.data() + ch * kTx11nPreamble;
        const int dl = 8 * ch, dh = 16 * ch;                                              // TCSD: 200 ns / 400 ns at 40 MHz
        for (int n = 0; n < 320; n++) o[n] = word(0, n - dl, 1);                          // L-STF
        for (int n = 0; n < 320; n++) o[320 + n] = word(1, n - 64 - dl, 1);               // L-LTF: GI2 of 64, two symbols
        for (int n = 0; n < 160; n++) o[640 + n] = word(0, n - 32 - dh, 1);               // HT-STF
        for (int n = 0; n < 160; n++) o[800 + n] = word(2, n - 32 - dh, 1);               // HT-LTF1
        for (int n = 0; n < 160; n++) o[960 + n] = word(2, n - 32 - dh, ch ? 1 : -1);     // HT-LTF2
    }
}

// the table on the device (sora_hip_tx11n and sora_hip_preamble11n): built once per device, complete before it is published
static int tx11n_preamble_ready(DevTables* D)
{
    std::lock_guard<std::mutex> lock(g_stage_mutex);
    if (!D->tx11n_preamble) {
        std::vector<uint32_t> tab; tx11n_preamble_host(tab);
        uint32_t* p = nullptr;
        HIPCHK(hipMalloc((void**)&p, tab.size() * sizeof(uint32_t)));
        const hipError_t e = hipMemcpy(p, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(p); return fail(SORA_ERR_HARDWARE_FAILED, "tx11n preamble upload", e); }
        D->tx11n_preamble = p; D->allocs.push_back(p);
    }
    return SORA_OK;
}

size_t sora_hip_tx11n_samples(uint32_t mpdu_len_nofcs, uint32_t mcs)
{
    Tx11nPlan P;
    if (!tx11n_plan(mpdu_len_nofcs, mcs, P)) return 0;
    return 1600 + 160 * (size_t)P.nsym;
}

int sora_hip_tx11n(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed,
                   size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, void* stream)
{
    if (sora_hip_device_count() <= 0) return fail(SORA_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
    if (!d_mpdu || !d_off || !d_len || !d_mcs || !d_out0 || !d_out1 || !d_out_off) return fail(SORA_ERR_INVALID_PARAM, "sora_hip_tx11n: null pointer");
    if (nframes == 0) return SORA_OK;
    DevTables* D = device_tables(); if (!D) return fail(SORA_ERR_HARDWARE_FAILED, "table upload failed");
    if (const int rc = tx11n_preamble_ready(D)) return rc;
    Tx11nArgs A{};
    A.mpdu = d_mpdu; A.off = d_off; A.len = d_len; A.mcs = d_mcs; A.seed = d_seed;
    A.out0 = reinterpret_cast<uint32_t*>(d_out0); A.out1 = reinterpret_cast<uint32_t*>(d_out1); A.out_off = d_out_off;
    A.preamble = D->tx11n_preamble; A.T = D->T;
    hipLaunchKernelGGL(k_tx11n, dim3((unsigned)nframes), dim3(256), 0, (hipStream_t)stream, A);
    HIPCHK(hipGetLastError());
    return SORA_OK;
}

// What sora_hip_preamble11n and sora_hip_preamble_ht40 share behind their own checks and their table: field 0 / 1 of both chains of a two-chain transmitter's table
// ([2][1120] samples), ncopies < kPreambleCopies times back to back
constexpr size_t kPreambleCopies = 1ull << 24;
static int preamble_copy(void (*kernel)(const uint4*, uint4*, uint4*, uint32_t, uint32_t, uint64_t), const char* name, const uint32_t* table, sora_complex16* d_out0,
                         sora_complex16* d_out1, int field, size_t ncopies, void* stream)
{
    const uint32_t w0 = field ? 160u : 0u, nw = field ? 120u : 160u;             // 16-byte words: samples 0..639 / 640..1119 of a chain's 1120
    const uint64_t nwords = (uint64_t)ncopies * nw;
    hipLaunchKernelGGL(kernel, dim3(stage_tiles(nwords, 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(table), reinterpret_cast<uint4*>(d_out0),
                       reinterpret_cast<uint4*>(d_out1), w0, nw, nwords);
    return launch_result(name);
}

// LSrc / HTSrc as a stage (the 802.11n modulation graph's other bricks: k_mod11n.hip): it copies the transmitter's table, so it stands here
int sora_hip_preamble11n(sora_complex16* d_out0, sora_complex16* d_out1, int field, size_t ncopies, void* stream)
{
    STAGE_ENTRY("sora_hip_preamble11n", !d_out0 || !d_out1, ncopies)
    if (field != 0 && field != 1) return fail(SORA_ERR_INVALID_PARAM, "sora_hip_preamble11n: field must be 0 (LSrc) or 1 (HTSrc)");
    STAGE_ALIGNED16("sora_hip_preamble11n", d_out0, d_out1)
    if (ncopies >= kPreambleCopies) return fail(SORA_ERR_CAPACITY, "sora_hip_preamble11n: too many copies for one call");
    DevTables* D = device_tables(); if (!D) return fail(SORA_ERR_HARDWARE_FAILED, "table upload failed");
    if (const int rc = tx11n_preamble_ready(D)) return rc;
    return preamble_copy(k_mod11n_preamble, "k_mod11n_preamble", D->tx11n_preamble, d_out0, d_out1, field, ncopies, stream);
}

// ---- 40 MHz HT 2x2 transmitter
size_t sora_hip_tx_ht40_samples(uint32_t mpdu_len_nofcs, uint32_t mcs)
{
    TxHt40Plan P;
    if (!tx_ht40_plan(mpdu_len_nofcs, mcs, P)) return 0;
    return 1280 + 160 * (2 + (size_t)P.nsym);
}

size_t sora_hip_tx_ht40_joint_samples(uint32_t mpdu_len_nofcs, uint32_t mcs)
{
    TxHt40Plan P;
    if (!tx_ht40_plan_joint(mpdu_len_nofcs, mcs, P)) return 0;
    return 1280 + 160 * (2 + (size_t)P.nsym);
}

size_t sora_hip_tx_ht40_gi_samples(uint32_t mpdu_len_nofcs, uint32_t mcs, uint32_t gi)
{
    TxHt40Plan P;
    if (gi > 1 || !tx_ht40_plan(mpdu_len_nofcs, mcs, P)) return 0;
    return tx_ht40_frame_samples(P.nsym, gi);
}

size_t sora_hip_tx_ht40_joint_gi_samples(uint32_t mpdu_len_nofcs, uint32_t mcs, uint32_t gi)
{
    TxHt40Plan P;
    if (gi > 1 || !tx_ht40_plan_joint(mpdu_len_nofcs, mcs, P)) return 0;
    return tx_ht40_frame_samples(P.nsym, gi);
}

size_t sora_hip_tx_ht40_mcs_samples(uint32_t mpdu_len_nofcs, uint32_t mcs, uint32_t gi, int mcs_max)
{
    TxHt40Plan P;
    if (gi > 1 || mcs_max < 0 || !tx_ht40_plan_mcs(mpdu_len_nofcs, mcs, (uint32_t)mcs_max, false, P)) return 0;
    return tx_ht40_frame_samples(P.nsym, gi);
}

size_t sora_hip_tx_ht40_joint_mcs_samples(uint32_t mpdu_len_nofcs, uint32_t mcs, uint32_t gi, int mcs_max)
{
    TxHt40Plan P;
    if (gi > 1 || mcs_max < 0 || !tx_ht40_plan_mcs(mpdu_len_nofcs, mcs, (uint32_t)mcs_max, true, P)) return 0;
    return tx_ht40_frame_samples(P.nsym, gi);
}

// the fixed fields through the same fixed-point IFFT as every other symbol (the four transmitters and sora_hip_preamble_ht40): built once per device, under the lock,
// and complete before it is published
static int tx_ht40_preamble_ready(DevTables* D, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(g_stage_mutex);
    if (!D->tx_ht40_preamble) {
        uint32_t* p = nullptr;
        HIPCHK(hipMalloc((void**)&p, 2 * kTxHt40Preamble * sizeof(uint32_t)));
        hipLaunchKernelGGL(k_tx_ht40_preamble, dim3(1), dim3(128), 0, st, p, D->T);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { (void)hipFree(p); return fail(SORA_ERR_HARDWARE_FAILED, "k_tx_ht40_preamble", e); }
        D->tx_ht40_preamble = p; D->allocs.push_back(p);
    }
    return SORA_OK;
}

// both codings: the per-stream one (two MPDUs and two seeds per frame) and the joint one (one of each).  guard: the _gi entry points, which launch the kernels that read
// a guard-interval kind per frame (d_gi; null: every frame long); the entry points without it launch the kernels they always launched
static int tx_ht40_launch(bool joint, const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed,
                          size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, void* stream, bool guard = false, const uint8_t* d_gi = nullptr,
                          bool mcs15 = false)
{
    if (sora_hip_device_count() <= 0) return fail(SORA_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
    if (!d_mpdu || !d_off || !d_len || !d_mcs || !d_out0 || !d_out1 || !d_out_off) return fail(SORA_ERR_INVALID_PARAM,
            guard ? (joint ? "sora_hip_tx_ht40_joint_gi: null pointer" : "sora_hip_tx_ht40_gi: null pointer") : joint ? "sora_hip_tx_ht40_joint: null pointer" :
            "sora_hip_tx_ht40: null pointer");
    if (nframes == 0) return SORA_OK;
    DevTables* D = device_tables(); if (!D) return fail(SORA_ERR_HARDWARE_FAILED, "table upload failed");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = tx_ht40_preamble_ready(D, st)) return rc;
    TxHt40Args A{};
    A.mpdu = d_mpdu; A.off = d_off; A.len = d_len; A.mcs = d_mcs; A.seed = d_seed;
    A.out0 = reinterpret_cast<uint32_t*>(d_out0); A.out1 = reinterpret_cast<uint32_t*>(d_out1); A.out_off = d_out_off;
    A.preamble = D->tx_ht40_preamble; A.T = D->T; A.gi = d_gi;
    if (mcs15) hipLaunchKernelGGL(joint ? k_tx_ht40_joint_mcs : k_tx_ht40_mcs, dim3((unsigned)nframes), dim3(256), 0, st, A);   // (the gate at 15: guard-aware too)
    else if (guard) hipLaunchKernelGGL(joint ? k_tx_ht40_joint_gi : k_tx_ht40_gi, dim3((unsigned)nframes), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(joint ? k_tx_ht40_joint : k_tx_ht40, dim3((unsigned)nframes), dim3(256), 0, st, A);
    HIPCHK(hipGetLastError());
    return SORA_OK;
}
int sora_hip_tx_ht40(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed,
                     size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, void* stream)
{
    return tx_ht40_launch(false, d_mpdu, d_off, d_len, d_mcs, d_seed, nframes, d_out0, d_out1, d_out_off, stream);
}
int sora_hip_tx_ht40_joint(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed,
                           size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, void* stream)
{
    return tx_ht40_launch(true, d_mpdu, d_off, d_len, d_mcs, d_seed, nframes, d_out0, d_out1, d_out_off, stream);
}
int sora_hip_tx_ht40_gi(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed, const uint8_t* d_gi,
                        size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, void* stream)
{
    return tx_ht40_launch(false, d_mpdu, d_off, d_len, d_mcs, d_seed, nframes, d_out0, d_out1, d_out_off, stream, true, d_gi);
}
int sora_hip_tx_ht40_joint_gi(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed, const uint8_t* d_gi,
                              size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, void* stream)
{
    return tx_ht40_launch(true, d_mpdu, d_off, d_len, d_mcs, d_seed, nframes, d_out0, d_out1, d_out_off, stream, true, d_gi);
}

// the _gi entry points behind a gate: 14 launches their kernels (the same bytes), 15 the kernels that accept MCS 15 as well
int sora_hip_tx_ht40_mcs(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed, const uint8_t* d_gi,
                         size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, int mcs_max, void* stream)
{
    if (mcs_max != 14 && mcs_max != 15) return fail(SORA_ERR_INVALID_PARAM, "sora_hip_tx_ht40_mcs: mcs_max is 14 or 15");
    return tx_ht40_launch(false, d_mpdu, d_off, d_len, d_mcs, d_seed, nframes, d_out0, d_out1, d_out_off, stream, true, d_gi, mcs_max == 15);
}
int sora_hip_tx_ht40_joint_mcs(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_mcs, const uint8_t* d_seed, const uint8_t* d_gi,
                               size_t nframes, sora_complex16* d_out0, sora_complex16* d_out1, const uint64_t* d_out_off, int mcs_max, void* stream)
{
    if (mcs_max != 14 && mcs_max != 15) return fail(SORA_ERR_INVALID_PARAM, "sora_hip_tx_ht40_joint_mcs: mcs_max is 14 or 15");
    return tx_ht40_launch(true, d_mpdu, d_off, d_len, d_mcs, d_seed, nframes, d_out0, d_out1, d_out_off, stream, true, d_gi, mcs_max == 15);
}

// the fixed fields as a stage (the 40 MHz HT modulation graph's other bricks: k_mod_ht40.hip): it copies the transmitters' table, so it stands here
int sora_hip_preamble_ht40(sora_complex16* d_out0, sora_complex16* d_out1, int field, size_t ncopies, void* stream)
{
    if (field != 0 && field != 1) return fail(SORA_ERR_INVALID_PARAM, "sora_hip_preamble_ht40: field must be 0 (L-STF, L-LTF) or 1 (HT-STF, HT-LTF1, HT-LTF2)");
    STAGE_ENTRY("sora_hip_preamble_ht40", !d_out0 || !d_out1, ncopies)
    STAGE_ALIGNED16("sora_hip_preamble_ht40", d_out0, d_out1)
    if (ncopies >= kPreambleCopies) return fail(SORA_ERR_CAPACITY, "sora_hip_preamble_ht40: too many copies for one call");
    DevTables* D = device_tables(); if (!D) return fail(SORA_ERR_HARDWARE_FAILED, "table upload failed");
    if (const int rc = tx_ht40_preamble_ready(D, (hipStream_t)stream)) return rc;
    return preamble_copy(k_mod_ht40_preamble, "k_mod_ht40_preamble", D->tx_ht40_preamble, d_out0, d_out1, field, ncopies, stream);
}

// ---- 802.11b transmitter
size_t sora_hip_tx11b_pre_samples(uint32_t mpdu_len_nofcs, uint32_t rate_kbps, uint32_t preamble)
{
    Tx11bPlan P;
    if (!tx11b_plan(mpdu_len_nofcs, rate_kbps, P, preamble)) return 0;
    return 4 * (size_t)P.nchips + 24;
}
size_t sora_hip_tx11b_samples(uint32_t mpdu_len_nofcs, uint32_t rate_kbps) { return sora_hip_tx11b_pre_samples(mpdu_len_nofcs, rate_kbps, 0); }

static int tx11b_launch(const char* who, const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps, const uint8_t* d_preamble,
                        const uint8_t* d_phase_in, uint8_t* d_phase_out, size_t nframes, int8_t* d_out, const uint64_t* d_out_off, void* stream)
{
    if (sora_hip_device_count() <= 0) return fail(SORA_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
    if (!d_mpdu || !d_off || !d_len || !d_rate_kbps || !d_out || !d_out_off) return fail(SORA_ERR_INVALID_PARAM, (std::string(who) + ": null pointer").c_str());
    if (nframes == 0) return SORA_OK;
    if (nframes > 0x7FFFFFFFu) return fail(SORA_ERR_INVALID_PARAM, (std::string(who) + ": too many frames for one call").c_str());
    DevTables* D = device_tables(); if (!D) return fail(SORA_ERR_HARDWARE_FAILED, "table upload failed");
    Tx11bArgs A{};
    A.mpdu = d_mpdu; A.off = d_off; A.len = d_len; A.rate = d_rate_kbps; A.phase_in = d_phase_in; A.phase_out = d_phase_out;
    A.out = d_out; A.out_off = d_out_off; A.T = D->T; A.preamble = d_preamble;
    // each frame's chips in G runs, one workgroup each, so that a small batch of long frames still fills the device
    const unsigned G = (unsigned)std::min<size_t>(64, std::max<size_t>(1, (2048 + nframes - 1) / nframes));
    hipLaunchKernelGGL(k_tx11b, dim3((unsigned)nframes, G), dim3(256), 0, (hipStream_t)stream, A);
    HIPCHK(hipGetLastError());
    return SORA_OK;
}
int sora_hip_tx11b(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps,
                   const uint8_t* d_phase_in, uint8_t* d_phase_out, size_t nframes, int8_t* d_out, const uint64_t* d_out_off, void* stream)
{
    return tx11b_launch("sora_hip_tx11b", d_mpdu, d_off, d_len, d_rate_kbps, nullptr, d_phase_in, d_phase_out, nframes, d_out, d_out_off, stream);
}
int sora_hip_tx11b_pre(const uint8_t* d_mpdu, const uint32_t* d_off, const uint32_t* d_len, const uint32_t* d_rate_kbps, const uint8_t* d_preamble,
                       const uint8_t* d_phase_in, uint8_t* d_phase_out, size_t nframes, int8_t* d_out, const uint64_t* d_out_off, void* stream)
{
    return tx11b_launch("sora_hip_tx11b_pre", d_mpdu, d_off, d_len, d_rate_kbps, d_preamble, d_phase_in, d_phase_out, nframes, d_out, d_out_off, stream);
}

// ---- capture ingest
size_t sora_hip_ingest_count(size_t raw_bytes, unsigned flags)
{
    uint64_t n;
    if (flags & SORA_INGEST_RXBLOCK) {                          // LoadSoraDumpFile (brickutil.h:40-55): a short last block gives what it holds
        const uint64_t full = raw_bytes / 128, rem = raw_bytes % 128;
        n = full * 28 + (rem > 16 ? std::min<uint64_t>(28, (rem - 16) / 4) : 0);
    } else n = raw_bytes / 4;
    if (flags & SORA_INGEST_44TO40) {                           // whole 28-sample blocks in, whole 28-sample blocks out (sampling.hpp:47-62)
        const uint64_t nin = n / 28 * 28;
        const uint64_t produced = nin - (nin + 9) / 11;         // every input except those with index % 11 == 1
        n = produced / 28 * 28;
    }
    if (flags & SORA_INGEST_DECIMATE2) n = n / 8 * 4;          // TDownSample2: bursts of 8 -> 4 (samples.hpp:9-47)
    return (size_t)n;
}

int sora_hip_ingest(const void* d_raw, size_t raw_bytes, unsigned flags, sora_complex16* d_out, size_t out_capacity, size_t* n_out, void* stream)
{
    if (sora_hip_device_count() <= 0) return fail(SORA_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
    if (!d_raw || !d_out || (flags & ~15u)) return fail(SORA_ERR_INVALID_PARAM, "sora_hip_ingest: bad argument");
    if (((uintptr_t)d_raw & 3) || ((uintptr_t)d_out & 3)) return fail(SORA_ERR_INVALID_PARAM, "sora_hip_ingest: buffers must be 4-byte aligned");
    const size_t n = sora_hip_ingest_count(raw_bytes, flags);
    if (n_out) *n_out = n;
    if (n > out_capacity) return fail(SORA_ERR_CAPACITY, "sora_hip_ingest: output buffer too small");
    if (n == 0) return SORA_OK;
    uint64_t done = 0;
    if ((flags & (SORA_INGEST_RXBLOCK | SORA_INGEST_44TO40)) == (SORA_INGEST_RXBLOCK | SORA_INGEST_44TO40) &&
        !((uintptr_t)d_raw & 15) && !((uintptr_t)d_out & 15)) {
        // whole tiles of 55 RX_BLOCKs -> 1400 (700 when decimating) samples through the LDS-staged kernel
        const uint64_t per_tile = (flags & SORA_INGEST_DECIMATE2) ? 700 : 1400;
        const uint64_t tiles = std::min<uint64_t>(raw_bytes / (55 * 128), n / per_tile);
        if (tiles) {
            hipLaunchKernelGGL(k_ingest_tile, dim3((unsigned)std::min<uint64_t>(tiles, 8 * 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)d_raw,
                    reinterpret_cast<uint32_t*>(d_out), flags, (uint32_t)tiles);
            done = tiles * per_tile;
        }
    }
    if (done < n)
        hipLaunchKernelGGL(k_ingest, dim3((unsigned)((n - done + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)d_raw,
                reinterpret_cast<uint32_t*>(d_out), done, (uint64_t)n, flags);
    HIPCHK(hipGetLastError());
    return SORA_OK;
}

// The stage works out of a caller-owned workspace (no allocation, no host wait).  Its layout, front to back:
//   head      the window-parallel trellis's code-rate list header (hdr[3]: this call's one list) and its proof record (4 kWinStatBanks counters)
//   soft      802.11a: every job's soft values packed to three bits each (k_soft_pack3: at byte ceil(off / 2), disjoint for any offsets and lengths because the
//             caller's ranges are); 802.11n: the caller's bytes as they are, at their own offsets (the trellis kernels read one byte past a stream's last value)
//   jobs      the job table
//   vecs      the window-parallel trellis's metric vectors (kWinVecBytes per unit, at most win_units(n) units)
// sora_hip_viterbi11a keeps the original signature on top of a grow-only workspace cached per device.
constexpr size_t kVitWsHdr = 0, kVitWsStats = 256, kVitWsHead = kVitWsStats + kWinStatsBytes;
static size_t vit_ws_round(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t vit_ws_packed_bytes(size_t soft_span_bytes) { return vit_ws_round(soft_span_bytes / 2 + 4 + kSoftSlack); }
static size_t vit_ws_bytes8(size_t soft_span_bytes) { return vit_ws_round(soft_span_bytes + kSoftSlack); }
static size_t vit_ws_tail(size_t n) { return vit_ws_round(sizeof(VitJob) * n) + (size_t)kWinVecBytes * win_vstride(n); }
size_t sora_hip_viterbi11a_workspace_bytes(size_t soft_span_bytes, size_t n)
{
    return kVitWsHead + vit_ws_packed_bytes(soft_span_bytes) + vit_ws_tail(n);
}
size_t sora_hip_viterbi11n_workspace_bytes(size_t soft_span_bytes, size_t n)
{
    return kVitWsHead + vit_ws_bytes8(soft_span_bytes) + vit_ws_tail(n);
}

// Both stage doors: check the arguments, make the soft streams and the job table in the workspace, then run the chosen trellis kernel over them.  WIN = 256: the
// 802.11a graph's T11aViterbi<5000*8,48,256,24>; WIN = 192: the 802.11n graph's T11aViterbi<5000*8,312,192,36>.
extern "C++" {
template <int WIN>
static int viterbi_ws(const char* name, const uint8_t* d_soft, size_t soft_span_bytes, const uint32_t* d_soft_off, const uint32_t* d_nsoft,
                      const uint16_t* d_frame_len, int code_rate, uint8_t* d_out, const uint32_t* d_out_off, size_t n, void* d_workspace, size_t workspace_bytes,
                      int lanes_per_pair, void* stream)
{
    const std::string nm(name);
    if (sora_hip_device_count() <= 0) return fail(SORA_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
    if (!d_soft || !d_soft_off || !d_nsoft || !d_frame_len || !d_out || !d_out_off || code_rate < 0 || code_rate > 2) return fail(SORA_ERR_INVALID_PARAM,
            (nm + ": bad argument").c_str());
    if (n == 0) return SORA_OK;
    TrellisChoice choice;
    if (!trellis_parse(lanes_per_pair, &choice)) return fail(SORA_ERR_INVALID_PARAM, (nm + ": lanes_per_pair is 0 (default: 64), 16, 64 or SORA_TRELLIS_WINDOWED").c_str());
    if (!d_workspace || ((uintptr_t)d_workspace & 15)) return fail(SORA_ERR_INVALID_PARAM, (nm + ": the workspace must be a 16-byte aligned device buffer").c_str());
    const size_t need = WIN == 256 ? sora_hip_viterbi11a_workspace_bytes(soft_span_bytes, n) : sora_hip_viterbi11n_workspace_bytes(soft_span_bytes, n);
    if (workspace_bytes < need) return fail(SORA_ERR_CAPACITY, (nm + ": workspace smaller than its _workspace_bytes()").c_str());
    if (soft_span_bytes >= (1ull << 32) || n >= (1ull << 31)) return fail(SORA_ERR_CAPACITY, (nm + ": batch too large").c_str());
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)d_workspace;
    uint32_t* hdr = (uint32_t*)(ws + kVitWsHdr);
    unsigned long long* stats = (unsigned long long*)(ws + kVitWsStats);
    uint8_t* soft = ws + kVitWsHead;
    VitJob* jobs = (VitJob*)(soft + (WIN == 256 ? vit_ws_packed_bytes(soft_span_bytes) : vit_ws_bytes8(soft_span_bytes)));
    uint16_t* vecs = (uint16_t*)((uint8_t*)jobs + vit_ws_round(sizeof(VitJob) * n));
    if (WIN == 256)
        hipLaunchKernelGGL(k_soft_pack3, dim3((unsigned)n), dim3(256), 0, st, d_soft, d_soft_off, d_nsoft, d_frame_len, d_out_off, code_rate, soft, jobs);
    else {
        HIPCHK(hipMemcpyAsync(soft, d_soft, soft_span_bytes, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_soft_jobs8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_soft_off, d_nsoft, d_frame_len, d_out_off, code_rate, (uint32_t)n, jobs);
    }
    const Trellis kind = choice.value_or(Trellis::Lanes64);
    const WinScratch W{ vecs, stats, win_vstride(n) };                           // (a view of the workspace: nothing is owned)
    if (kind == Trellis::Windowed) {
        // the receive path's own unit plan over one code-rate list of n frames: the batch size decides the units' geometry (dev_winplan.h)
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)hdr, 0, 4, st));
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)hdr, (int)n, 1, st));
        HIPCHK(hipMemsetAsync(stats, 0, kWinStatsBytes, st));
    }
    trellis_launch<WIN>(kind, trellis_single(jobs, hdr, (uint32_t)n, WIN == 256), soft, d_out, st, W);
    HIPCHK(hipGetLastError());
    return SORA_OK;
}
}  // extern "C++"

int sora_hip_viterbi11a_ws(const uint8_t* d_soft, size_t soft_span_bytes, const uint32_t* d_soft_off, const uint32_t* d_nsoft, const uint16_t* d_frame_len,
                           int code_rate, uint8_t* d_out, const uint32_t* d_out_off, size_t n, void* d_workspace, size_t workspace_bytes, int lanes_per_pair, void* stream)
{
    return viterbi_ws<256>("sora_hip_viterbi11a_ws", d_soft, soft_span_bytes, d_soft_off, d_nsoft, d_frame_len, code_rate, d_out, d_out_off, n, d_workspace,
                           workspace_bytes, lanes_per_pair, stream);
}
int sora_hip_viterbi11n_ws(const uint8_t* d_soft, size_t soft_span_bytes, const uint32_t* d_soft_off, const uint32_t* d_nsoft, const uint16_t* d_frame_len,
                           int code_rate, uint8_t* d_out, const uint32_t* d_out_off, size_t n, void* d_workspace, size_t workspace_bytes, int lanes_per_pair, void* stream)
{
    return viterbi_ws<192>("sora_hip_viterbi11n_ws", d_soft, soft_span_bytes, d_soft_off, d_nsoft, d_frame_len, code_rate, d_out, d_out_off, n, d_workspace,
                           workspace_bytes, lanes_per_pair, stream);
}

int sora_hip_viterbi_window_stats(const void* d_workspace, unsigned long long out[4], void* stream)
{
    if (!d_workspace || !out) return fail(SORA_ERR_INVALID_PARAM, "sora_hip_viterbi_window_stats: null argument");
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < 4; i++) out[i] = 0;
    return win_stats_add((const unsigned long long*)((const uint8_t*)d_workspace + kVitWsStats), st, out);
}

namespace {
struct VitWs { void* p = nullptr; size_t bytes = 0; };
std::mutex g_vitws_mutex;
VitWs g_vitws[64];
}

int sora_hip_viterbi11a(const uint8_t* d_soft, const uint32_t* d_soft_off, const uint32_t* d_nsoft, const uint16_t* d_frame_len,
                        int code_rate, uint8_t* d_out, const uint32_t* d_out_off, size_t n, void* stream)
{
    if (sora_hip_device_count() <= 0) return fail(SORA_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
    if (!d_soft || !d_soft_off || !d_nsoft || !d_frame_len || !d_out || !d_out_off || code_rate < 0 || code_rate > 2) return fail(SORA_ERR_INVALID_PARAM,
            "sora_hip_viterbi11a: bad argument");
    if (n == 0) return SORA_OK;
    hipStream_t st = (hipStream_t)stream;
    // This signature does not say how far the soft buffer reaches: read the extent back once (the _ws entry point takes it as an argument).
    std::vector<uint32_t> h_off(n), h_nsoft(n);
    HIPCHK(hipMemcpyAsync(h_off.data(), d_soft_off, 4 * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_nsoft.data(), d_nsoft, 4 * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t span = 0;
    for (size_t i = 0; i < n; i++) {
        if (h_nsoft[i] < 24) return fail(SORA_ERR_INVALID_PARAM, "sora_hip_viterbi11a: a job needs at least one OFDM symbol of soft values");
        span = std::max<uint64_t>(span, (uint64_t)h_off[i] + h_nsoft[i]);
    }
    if (span >> 32) return fail(SORA_ERR_CAPACITY, "sora_hip_viterbi11a: batch too large");
    int dev = 0; HIPCHK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(SORA_ERR_INVALID_PARAM, "sora_hip_viterbi11a: device ordinal out of range");
    const size_t need = sora_hip_viterbi11a_workspace_bytes((size_t)span, n);
    std::lock_guard<std::mutex> lock(g_vitws_mutex);                             // one cached workspace per device: calls through this signature are serialised
    VitWs& W = g_vitws[dev];
    if (W.bytes < need) {
        if (W.p) { HIPCHK(hipDeviceSynchronize()); (void)hipFree(W.p); W.p = nullptr; W.bytes = 0; }
        HIPCHK(hipMalloc(&W.p, need + need / 4));
        W.bytes = need + need / 4;
    }
    const int rc = sora_hip_viterbi11a_ws(d_soft, (size_t)span, d_soft_off, d_nsoft, d_frame_len, code_rate, d_out, d_out_off, n, W.p, W.bytes, 0, stream);
    if (rc != SORA_OK) return rc;
    HIPCHK(hipStreamSynchronize(st));                                             // the cached workspace is free for the next call when this one returns
    return SORA_OK;
}

}  // extern "C"
