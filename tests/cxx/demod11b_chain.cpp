// demod11b_chain.cpp -- the byte paths of the 802.11b receive graph built from the adapters of include/sora_brick.hpp and EXECUTED on the GPU
// (tests/test_gpu_11b_stage_hosts.py), sink first and in the order of kernel/bb/demod11/fb11bdemod_config.hpp:122-172:
//   1 Mbps:    source pin -> THip11bDespread<8> -> THip11bDBPSKDemap<1> -+
//   2 Mbps:    source pin -> THip11bDespread<4> -> THip11bDQPSKDemap<1> -+-> THip11bDesc741<1> -> sink
//   5.5 Mbps:  source pin -> THip11bCCK5P5Decoder<1> --------------------+
//   11 Mbps:   source pin -> THip11bCCK11Decoder<1> ---------------------+
// One byte per burst, so last_symbol, byte_reg and is_even all cross burst boundaries, in the one device record the adapters share (the graph's context).  The host
// plays what is in front: the chips of a frame's payload come from a file, the record starts as the bricks in front left it.
// usage: demod11b_chain <1|2|5|11> <chips.bin> <last_symbol word> <byte_reg> <out.bin>      chips.bin: COMPLEX16; out.bin: the descrambled bytes
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sora_brick.hpp"

using namespace sora_brick;

// the sink: appends every burst to a host vector
class TCollect {
public:
    TCollect(CF_Error&, std::vector<uint8_t>& host) : host_(host) {}
    void Reset() {}
    void Flush() {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            uint8_t b;
            if (sora_hip_stream_synchronize(nullptr) != SORA_OK || sora_hip_memcpy_d2h(&b, ipin.peek(), 1) != SORA_OK) return false;
            host_.push_back(b);
            ipin.pop();
        }
        return true;
    }
private:
    std::vector<uint8_t>& host_;
};

template <class T> static T* dmalloc(size_t count)
{
    T* p = (T*)sora_hip_malloc(count * sizeof(T));
    if (!p) { fprintf(stderr, "device memory: %s\n", sora_hip_last_error()); exit(1); }
    return p;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s failed: error_code %08x (%s)\n", #x, ctx.error_code, sora_hip_last_error()); return 1; } } while (0)

// feed `first` burst by burst
template <size_t BURST, class FIRST>
static int feed(CF_Error& ctx, FIRST& first, const std::vector<sora_complex16>& chips, sora_complex16* d_in)
{
    DevicePin<sora_complex16, BURST> src(d_in);
    first.Reset();
    for (size_t at = 0; at + BURST <= chips.size(); at += BURST) {
        CHECK(sora_hip_stream_synchronize(nullptr) == SORA_OK);                            // (the pin's buffer is rewritten: one burst in flight)
        CHECK(sora_hip_memcpy_h2d(src.append(), chips.data() + at, BURST * sizeof(sora_complex16)) == SORA_OK);
        CHECK(first.Process(src));
    }
    first.Flush();
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 6) { fprintf(stderr, "usage: %s <1|2|5|11> <chips.bin> <last_symbol word> <byte_reg> <out.bin>\n", argv[0]); return 2; }
    const int kind = atoi(argv[1]);
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 1;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<sora_complex16> chips((size_t)bytes / sizeof(sora_complex16));
    if (fread(chips.data(), sizeof(sora_complex16), chips.size(), f) != chips.size()) return 1;
    fclose(f);

    CF_Error ctx;
    std::vector<uint8_t> host;
    sora_stream11b_state st{};
    const uint32_t last = (uint32_t)strtoul(argv[3], nullptr, 0);
    st.last_symbol.re = (int16_t)(last & 0xFFFF); st.last_symbol.im = (int16_t)(last >> 16); st.byte_reg = (uint32_t)strtoul(argv[4], nullptr, 0);
    st.is_even = 1;                                                                        // (TCCK11Decoder's Reset has to clear it)
    sora_stream11b_state* d_st = dmalloc<sora_stream11b_state>(1);
    CHECK(sora_hip_memcpy_h2d(d_st, &st, sizeof(st)) == SORA_OK);
    sora_complex16* d_in = dmalloc<sora_complex16>(11 * 8);
    sora_complex16* d_sym = dmalloc<sora_complex16>(8);
    uint8_t* d_raw = dmalloc<uint8_t>(16); uint8_t* d_out = dmalloc<uint8_t>(16);
    uint8_t* d_tabs = dmalloc<uint8_t>(64);

    TCollect sink(ctx, host);
    THip11bDesc741<1, CF_Error, TCollect> desc(ctx, &sink, d_out, d_tabs, d_st);
    int rc = 2;
    if (kind == 1) {
        THip11bDBPSKDemap<1, CF_Error, decltype(desc)> demap(ctx, &desc, d_raw, d_tabs + 16, d_st);
        THip11bDespread<8, CF_Error, decltype(demap)> despread(ctx, &demap, d_sym, d_tabs + 32);
        rc = feed<11 * 8>(ctx, despread, chips, d_in);
    } else if (kind == 2) {
        THip11bDQPSKDemap<1, CF_Error, decltype(desc)> demap(ctx, &desc, d_raw, d_tabs + 16, d_st);
        THip11bDespread<4, CF_Error, decltype(demap)> despread(ctx, &demap, d_sym, d_tabs + 32);
        rc = feed<11 * 4>(ctx, despread, chips, d_in);
    } else if (kind == 5) {
        THip11bCCK5P5Decoder<1, CF_Error, decltype(desc)> cck(ctx, &desc, d_raw, d_tabs + 16, d_st);
        rc = feed<16>(ctx, cck, chips, d_in);
    } else if (kind == 11) {
        THip11bCCK11Decoder<1, CF_Error, decltype(desc)> cck(ctx, &desc, d_raw, d_tabs + 16, d_st);
        rc = feed<8>(ctx, cck, chips, d_in);
    }
    if (rc) return rc;
    FILE* fo = fopen(argv[5], "wb");
    if (!fo || fwrite(host.data(), 1, host.size(), fo) != host.size()) return 1;
    fclose(fo);
    printf("demod11b chain: %zu chips in, %zu bytes out\n", chips.size(), host.size());
    return 0;
}
