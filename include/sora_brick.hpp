// sora_brick.hpp -- BRICK-shaped adapters over the C ABI of sora_hip.h.
//
// The reference's operator API is the compile-time BRICK protocol (kernel/brick/inc/brick.h:151-475):
// a brick declares DEFINE_IPORT(TYPE,BURST)/DEFINE_OPORT(TYPE,BURST), implements
//     template<class T_IPIN> bool Process(T_IPIN& ipin)   -- while(ipin.check_read()){peek; append; pop; Next()->Process(opin());}
// plus Reset() and Flush(), and reports errors through bool + CF_Error::error_code.
// These adapters keep exactly that shape -- same verbs, same port TYPEs, burst = 64*N / 48*N_BPSC*N soft values
// for a batch of N symbols -- so a graph built with CREATE_BRICK_* can put `THipFFT64<N>` where `TFFT64`
// (kernel/bb/Brick11/src/fft.hpp:108-135) sits.  The pin-queue contract is reduced to the three calls the
// reference's idiom uses (check_read / peek / pop on the input pin, append on the output pin): any TPinQueue
// (kernel/brick/inc/pinqueue.h:104-183) satisfies it.  The queue buffers must be HBM-resident (device pointers):
// the adapters move no data across PCIe.
//
// Header-only, C++17, no dependency beyond sora_hip.h; nothing here is required by the C host path.
#pragma once
#include <cstddef>
#include <cstdint>
#include "sora_hip.h"

namespace sora_brick {

struct CF_Error { uint32_t error_code = 0; };                 // kernel/brick/inc/stdfacade.h:14-18

template <class TYPE, size_t BURST> struct port_traits { using type = TYPE; static constexpr size_t burst = BURST; };

// Minimal device-resident pin: one burst in flight (the N:N specialisation of TPinQueue, pinqueue.h:152-183).
template <class T, size_t BURST>
class DevicePin {
public:
    explicit DevicePin(T* d_buf = nullptr) : buf_(d_buf), cnt_(0) {}
    void bind(T* d_buf) { buf_ = d_buf; }
    bool check_read() const { return cnt_ > 0; }
    const T* peek() const { return buf_; }
    void pop() { cnt_ = 0; }
    T* append() { cnt_ = BURST; return buf_; }
    void clear() { cnt_ = 0; }
private:
    T* buf_; size_t cnt_;
};

// Common part of a filter brick: next-brick pointer, context, stream.
template <class T_CTX, class T_NEXT>
class HipFilter {
public:
    HipFilter(T_CTX& ctx, T_NEXT* next, void* stream = nullptr) : ctx_(ctx), next_(next), stream_(stream) {}
    void Reset() { if (next_) next_->Reset(); }
    void Flush() { if (next_) next_->Flush(); }
protected:
    bool raise(int rc) { if (rc != SORA_OK) { ctx_.error_code = (uint32_t)rc; return false; } return true; }
    T_CTX& ctx_; T_NEXT* next_; void* stream_;
};

// TFFT64 (fft.hpp:108-135): IPORT COMPLEX16 x 64  ->  OPORT COMPLEX16 x 64, batched over N symbols.
template <size_t N, class T_CTX, class T_NEXT>
class THipFFT64 : public HipFilter<T_CTX, T_NEXT> {
public:
    using iport_traits = port_traits<sora_complex16, 64 * N>;
    using oport_traits = port_traits<sora_complex16, 64 * N>;
    THipFFT64(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* stream = nullptr)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, stream), opin_(d_out) {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            const sora_complex16* in = ipin.peek();
            sora_complex16* out = opin_.append();
            if (!this->raise(sora_hip_fft64(in, out, N, this->stream_))) return false;
            ipin.pop();
            if (this->next_ && !this->next_->Process(opin_)) return false;
        }
        return true;
    }
    DevicePin<sora_complex16, 64 * N>& opin() { return opin_; }
private:
    DevicePin<sora_complex16, 64 * N> opin_;
};

// T11aDemap<N_BPSC>::Filter (demapper11a.hpp:10-79): IPORT COMPLEX16 x 64 -> OPORT uchar x 48*N_BPSC.
template <int N_BPSC, size_t N, class T_CTX, class T_NEXT>
class THip11aDemap : public HipFilter<T_CTX, T_NEXT> {
public:
    using iport_traits = port_traits<sora_complex16, 64 * N>;
    using oport_traits = port_traits<uint8_t, 48 * N_BPSC * N>;
    THip11aDemap(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* stream = nullptr)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, stream), opin_(d_out) {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            uint8_t* out = opin_.append();
            if (!this->raise(sora_hip_demap11a(ipin.peek(), out, N_BPSC, N, this->stream_))) return false;
            ipin.pop();
            if (this->next_ && !this->next_->Process(opin_)) return false;
        }
        return true;
    }
    DevicePin<uint8_t, 48 * N_BPSC * N>& opin() { return opin_; }
private:
    DevicePin<uint8_t, 48 * N_BPSC * N> opin_;
};

// T11aDeinterleave{BPSK,QPSK,QAM16,QAM64} (deinterleaver.hpp): IPORT uchar x N_CBPS -> OPORT uchar x N_CBPS.
template <int N_BPSC, size_t N, class T_CTX, class T_NEXT>
class THip11aDeinterleave : public HipFilter<T_CTX, T_NEXT> {
public:
    using iport_traits = port_traits<uint8_t, 48 * N_BPSC * N>;
    using oport_traits = port_traits<uint8_t, 48 * N_BPSC * N>;
    THip11aDeinterleave(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* stream = nullptr)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, stream), opin_(d_out) {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            uint8_t* out = opin_.append();
            if (!this->raise(sora_hip_deinterleave11a(ipin.peek(), out, N_BPSC, N, this->stream_))) return false;
            ipin.pop();
            if (this->next_ && !this->next_->Process(opin_)) return false;
        }
        return true;
    }
    DevicePin<uint8_t, 48 * N_BPSC * N>& opin() { return opin_; }
private:
    DevicePin<uint8_t, 48 * N_BPSC * N> opin_;
};

// TSink that terminates a test graph (TDropAny analogue).
template <class T_CTX>
class TDrop {
public:
    explicit TDrop(T_CTX&) {}
    void Reset() {}
    void Flush() {}
    template <class T_IPIN> bool Process(T_IPIN& ipin) { while (ipin.check_read()) ipin.pop(); return true; }
};

// TDownSample44_40 (sampling.hpp:35-66) / TDownSample2 (samples.hpp:9-47) as one filter over a whole capture: the
// input pin holds NIN COMPLEX16 (a multiple of 28), the output pin what sora_hip_ingest_count says comes out of it.
template <size_t NIN, unsigned FLAGS, class T_CTX, class T_NEXT>
class THipResample : public HipFilter<T_CTX, T_NEXT> {
    static_assert(NIN % 28 == 0 && !(FLAGS & SORA_INGEST_RXBLOCK), "whole RX blocks of plain samples");
public:
    static constexpr size_t NOUT = NIN;                          // capacity; the produced count is returned by produced()
    using iport_traits = port_traits<sora_complex16, NIN>;
    using oport_traits = port_traits<sora_complex16, NOUT>;
    THipResample(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* stream = nullptr)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, stream), opin_(d_out) {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            sora_complex16* out = opin_.append();
            if (!this->raise(sora_hip_ingest(ipin.peek(), NIN * sizeof(sora_complex16), FLAGS, out, NOUT, &produced_, this->stream_))) return false;
            ipin.pop();
            if (this->next_ && !this->next_->Process(opin_)) return false;
        }
        return true;
    }
    size_t produced() const { return produced_; }
    DevicePin<sora_complex16, NOUT>& opin() { return opin_; }
private:
    DevicePin<sora_complex16, NOUT> opin_;
    size_t produced_ = 0;
};

// ------------------------------------------------------------------------------------------------
// The remaining stage bricks.  They all have the shape spelt out above (peek / append / call / pop / Next()->Process), so they are
// one template: IPORT IT x IB -> OPORT OT x OB with the C entry point supplied as a callable `int(const IT*, OT*, void* stream)`.
template <class IT, size_t IB, class OT, size_t OB, class CALL, class T_CTX, class T_NEXT>
class THipStage : public HipFilter<T_CTX, T_NEXT> {
public:
    using iport_traits = port_traits<IT, IB>;
    using oport_traits = port_traits<OT, OB>;
    THipStage(T_CTX& ctx, T_NEXT* next, OT* d_out, CALL call, void* stream = nullptr)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, stream), opin_(d_out), call_(call) {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            OT* out = opin_.append();
            if (!this->raise(call_(ipin.peek(), out, this->stream_))) return false;
            ipin.pop();
            if (this->next_ && !this->next_->Process(opin_)) return false;
        }
        return true;
    }
    DevicePin<OT, OB>& opin() { return opin_; }
private:
    DevicePin<OT, OB> opin_; CALL call_;
};

// FFT<128> (core/inc/fft_r4dif.h): IPORT COMPLEX16 x 128 -> OPORT COMPLEX16 x 128, N transforms per burst.
struct CallFFT128 { size_t n; int operator()(const sora_complex16* in, sora_complex16* out, void* st) const { return sora_hip_fft128(in, out, n, st); } };
template <size_t N, class T_CTX, class T_NEXT>
struct THipFFT128 : THipStage<sora_complex16, 128 * N, sora_complex16, 128 * N, CallFFT128, T_CTX, T_NEXT> {
    THipFFT128(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 128 * N, sora_complex16, 128 * N, CallFFT128, T_CTX, T_NEXT>(ctx, next, d_out, CallFFT128{ N }, stream) {}
};

// T11aLTS (channel_11a.hpp:33-230): IPORT COMPLEX16 x 144.  The reference brick is a sink that fills the context facades
// CF_CFOffset / CF_FreqCompensate / CF_Channel_11a; here they are the device record `d_ctx` (sora_lts11a_ctx) the later bricks are bound to.
template <class T_CTX>
class THip11aLTS {
public:
    using iport_traits = port_traits<sora_complex16, 144>;
    THip11aLTS(T_CTX& ctx, sora_lts11a_ctx* d_ctx, void* stream = nullptr) : ctx_(ctx), d_ctx_(d_ctx), stream_(stream) {}
    void Reset() {}
    void Flush() {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            const int rc = sora_hip_lts11a(ipin.peek(), d_ctx_, 1, stream_);
            if (rc != SORA_OK) { ctx_.error_code = (uint32_t)rc; return false; }
            ipin.pop();
        }
        return true;
    }
private:
    T_CTX& ctx_; sora_lts11a_ctx* d_ctx_; void* stream_;
};

// T11aDataSymbol -> TFreqCompensation -> TFFT64 -> TChannelEqualization (PHY_11a.hpp:361-430, channel_11a.hpp:532-653) as one brick:
// IPORT COMPLEX16 x 80 -> OPORT COMPLEX16 x 64, N symbols per burst, bound to the frame's T11aLTS record.
struct CallSymFront11a { const sora_lts11a_ctx* d_ctx; size_t n; int operator()(const sora_complex16* in, sora_complex16* out,
        void* st) const { return sora_hip_symfront11a(in, d_ctx, nullptr, out, n, st); } };
template <size_t N, class T_CTX, class T_NEXT>
struct THip11aSymFront : THipStage<sora_complex16, 80 * N, sora_complex16, 64 * N, CallSymFront11a, T_CTX, T_NEXT> {
    THip11aSymFront(T_CTX& ctx, T_NEXT* next, const sora_lts11a_ctx* d_ctx, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 80 * N, sora_complex16, 64 * N, CallSymFront11a, T_CTX, T_NEXT>(ctx, next, d_out, CallSymFront11a{ d_ctx, N }, stream) {}
};

// The three one-multiply bricks of the symbol chain, each where its SSE brick sits (IPORT COMPLEX16 x 64 -> OPORT COMPLEX16 x 64, N symbols per burst):
//   THipFreqCompensation     TFreqCompensation     (channel_11a.hpp:614-653)   bound to the frame's T11aLTS record (CF_FreqCompensate::Coeffs)
//   THipChannelEqualization  TChannelEqualization  (channel_11a.hpp:534-604)   bound to the same record (CF_Channel_11a::ChannelCoeffs)
//   THipPhaseCompensate      TPhaseCompensate      (freqoffset.hpp:16-66)      bound to the tracker's state (CF_PhaseCompensate::CompCoeffs = sora_track11a_state::comp)
struct CallFreqComp11a { const sora_lts11a_ctx* d_ctx; size_t n; int operator()(const sora_complex16* in, sora_complex16* out,
        void* st) const { return sora_hip_freq_comp11a(in, d_ctx, nullptr, out, n, st); } };
struct CallEqualize11a { const sora_lts11a_ctx* d_ctx; size_t n; int operator()(const sora_complex16* in, sora_complex16* out,
        void* st) const { return sora_hip_equalize11a(in, d_ctx, nullptr, out, n, st); } };
struct CallPhaseComp11a { const sora_track11a_state* d_state; size_t n; int operator()(const sora_complex16* in, sora_complex16* out,
        void* st) const { return sora_hip_phase_comp11a(in, d_state, nullptr, out, n, st); } };
template <size_t N, class T_CTX, class T_NEXT>
struct THipFreqCompensation : THipStage<sora_complex16, 64 * N, sora_complex16, 64 * N, CallFreqComp11a, T_CTX, T_NEXT> {
    THipFreqCompensation(T_CTX& ctx, T_NEXT* next, const sora_lts11a_ctx* d_ctx, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 64 * N, sora_complex16, 64 * N, CallFreqComp11a, T_CTX, T_NEXT>(ctx, next, d_out, CallFreqComp11a{ d_ctx, N }, stream) {}
};
template <size_t N, class T_CTX, class T_NEXT>
struct THipChannelEqualization : THipStage<sora_complex16, 64 * N, sora_complex16, 64 * N, CallEqualize11a, T_CTX, T_NEXT> {
    THipChannelEqualization(T_CTX& ctx, T_NEXT* next, const sora_lts11a_ctx* d_ctx, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 64 * N, sora_complex16, 64 * N, CallEqualize11a, T_CTX, T_NEXT>(ctx, next, d_out, CallEqualize11a{ d_ctx, N }, stream) {}
};
template <size_t N, class T_CTX, class T_NEXT>
struct THipPhaseCompensate : THipStage<sora_complex16, 64 * N, sora_complex16, 64 * N, CallPhaseComp11a, T_CTX, T_NEXT> {
    THipPhaseCompensate(T_CTX& ctx, T_NEXT* next, const sora_track11a_state* d_state, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 64 * N, sora_complex16, 64 * N, CallPhaseComp11a, T_CTX, T_NEXT>(ctx, next, d_out, CallPhaseComp11a{ d_state, N }, stream) {}
};

// TPhaseCompensate -> TPilotTrack (freqoffset.hpp:14-66, pilot.hpp:121-269): IPORT COMPLEX16 x 64 -> OPORT COMPLEX16 x 64, N symbols of ONE
// frame per burst; CF_PhaseCompensate / CF_PilotTrack live in `d_state` and carry over from burst to burst.  d_first / d_nsym: device words
// holding 0 and N (the C entry point takes frame tables).
struct CallPilotTrack11a {
    const uint32_t* d_first; const uint32_t* d_nsym; sora_track11a_state* d_state;
    int operator()(const sora_complex16* in, sora_complex16* out, void* st) const { return sora_hip_pilot_track11a(in, d_first, d_nsym, d_state, out, 1, st); }
};
template <size_t N, class T_CTX, class T_NEXT>
struct THip11aPilotTrack : THipStage<sora_complex16, 64 * N, sora_complex16, 64 * N, CallPilotTrack11a, T_CTX, T_NEXT> {
    THip11aPilotTrack(T_CTX& ctx, T_NEXT* next, const uint32_t* d_first, const uint32_t* d_nsym, sora_track11a_state* d_state, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 64 * N, sora_complex16, 64 * N, CallPilotTrack11a, T_CTX, T_NEXT>(ctx, next, d_out, CallPilotTrack11a{ d_first, d_nsym, d_state }, stream) {}
};

// T11aViterbi<5000*8,48,256,24> (viterbi.hpp:103-237): IPORT uchar x 48*N_BPSC (one symbol's soft values) -> OPORT uchar x frame_length + 2.
// Like the reference brick it consumes symbol bursts and knows the frame from the context (SetFrame = CF_11aRxVector: length, code rate,
// symbols); the trellis is run when the last symbol has arrived.  d_frame: device scratch of nsym x 48*N_BPSC soft values + 16 bytes of tables.
template <int N_BPSC, class T_CTX, class T_NEXT>
class THip11aViterbi : public HipFilter<T_CTX, T_NEXT> {
public:
    using iport_traits = port_traits<uint8_t, 48 * N_BPSC>;
    THip11aViterbi(T_CTX& ctx, T_NEXT* next, uint8_t* d_frame, uint8_t* d_out, void* stream = nullptr)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, stream), d_soft_(d_frame + 16), d_tab_(d_frame), d_out_(d_out) {}
    void SetFrame(uint16_t frame_length, int code_rate, uint32_t nsym) { len_ = frame_length; cr_ = code_rate; nsym_ = nsym; got_ = 0; }
    void Reset() { got_ = 0; HipFilter<T_CTX, T_NEXT>::Reset(); }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            if (got_ < nsym_ && sora_hip_memcpy_d2d(d_soft_ + (size_t)got_ * 48 * N_BPSC, ipin.peek(), 48 * N_BPSC,
                    this->stream_) != SORA_OK) return this->raise(SORA_ERR_HARDWARE_FAILED);
            ipin.pop();
            if (++got_ == nsym_) {
                const uint32_t tab[4] = { 0u, nsym_ * 48u * (uint32_t)N_BPSC, (uint32_t)len_, 0u };   // soft_off, nsoft, frame_len (uint16), out_off
                if (sora_hip_memcpy_h2d(d_tab_, tab, sizeof(tab)) != SORA_OK) return this->raise(SORA_ERR_HARDWARE_FAILED);
                const uint32_t* t = reinterpret_cast<const uint32_t*>(d_tab_);
                if (!this->raise(sora_hip_viterbi11a(d_soft_, t, t + 1, reinterpret_cast<const uint16_t*>(t + 2), cr_, d_out_, t + 3, 1, this->stream_))) return false;
                decoded_ = true;
            }
        }
        return true;
    }
    bool decoded() const { return decoded_; }
    const uint8_t* output() const { return d_out_; }
private:
    uint8_t* d_soft_; uint8_t* d_tab_; uint8_t* d_out_;
    uint16_t len_ = 0; int cr_ = 0; uint32_t nsym_ = 0, got_ = 0; bool decoded_ = false;
};

// 802.11n stage bricks (one burst = N symbols / frames), each forwarding to its entry point:
//   T11nDemap* (demapper11n.hpp:89-309), T11nDeinterleave*_S0/_S1 (deinterleaver_11n.hpp), TMimoChannelComp (channel_11n.hpp:445-521)
struct CallDemap11n { int nb; size_t n; int operator()(const sora_complex16* in, uint8_t* out, void* st) const { return sora_hip_demap11n(in, out, nb, n, st); } };
template <int N_BPSC, size_t N, class T_CTX, class T_NEXT>
struct THip11nDemap : THipStage<sora_complex16, 64 * N, uint8_t, 52 * N_BPSC * N, CallDemap11n, T_CTX, T_NEXT> {
    THip11nDemap(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 64 * N, uint8_t, 52 * N_BPSC * N, CallDemap11n, T_CTX, T_NEXT>(ctx, next, d_out, CallDemap11n{ N_BPSC, N }, stream) {}
};
struct CallDeint11n { int nb, ss; size_t n; int operator()(const uint8_t* in, uint8_t* out, void* st) const { return sora_hip_deinterleave11n(in, out, nb, ss, n, st); } };
template <int N_BPSC, int SPATIAL_STREAM, size_t N, class T_CTX, class T_NEXT>
struct THip11nDeinterleave : THipStage<uint8_t, 52 * N_BPSC * N, uint8_t, 52 * N_BPSC * N, CallDeint11n, T_CTX, T_NEXT> {
    THip11nDeinterleave(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* stream = nullptr)
        : THipStage<uint8_t, 52 * N_BPSC * N, uint8_t, 52 * N_BPSC * N, CallDeint11n, T_CTX, T_NEXT>(ctx, next, d_out, CallDeint11n{ N_BPSC, SPATIAL_STREAM, N }, stream) {}
};
// TMimoChannelComp: NSTREAM = 2 ports in the reference (two RX chains in, two spatial streams out); here the two streams are the two halves of
// one burst: IPORT COMPLEX16 x 2 x 64N (chain 0 symbols, then chain 1) -> OPORT COMPLEX16 x 2 x 64N (stream 0, then stream 1).
struct CallMimoComp11n {
    const sora_complex16* d_hinv; size_t n;
    int operator()(const sora_complex16* in, sora_complex16* out, void* st) const { return sora_hip_mimo_comp11n(d_hinv, nullptr, in, in + 64 * n, out, out + 64 * n, n, st); }
};
template <size_t N, class T_CTX, class T_NEXT>
struct THip11nMimoComp : THipStage<sora_complex16, 128 * N, sora_complex16, 128 * N, CallMimoComp11n, T_CTX, T_NEXT> {
    THip11nMimoComp(T_CTX& ctx, T_NEXT* next, const sora_complex16* d_hinv, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 128 * N, sora_complex16, 128 * N, CallMimoComp11n, T_CTX, T_NEXT>(ctx, next, d_out, CallMimoComp11n{ d_hinv, N }, stream) {}
};

// ------------------------------------------------------------------------------------------------
// The bricks of the 802.11a modulation graph (kernel/bb/demod11/fb11amod_config.hpp:74-109), each where its SSE brick sits.  Port TYPEs as in the reference, one burst =
// N symbols (the byte-wide bricks: the bytes of N symbols, a whole number of the brick's own bursts).  The stateless ones are THipStage; the scrambler, the encoder and
// the pilot brick keep their frame state from Process to Process and clear it in Reset, as the bricks do.  Their frame tables are device words the caller provides.

// T11aSc (scramble.hpp:170-261): IPORT uchar x NBYTES -> OPORT uchar x NBYTES.  CF_ScramblerSeed = SetSeed, CF_ScramblerControl = SetTail: the byte of the frame (counted
// from the last Reset) that goes through TAIL_SCRAMBLE, every other byte DO_SCRAMBLE.  The register is kept on the host: a byte's mask is a function of the register and
// the byte's index alone, so it is advanced without looking at the data.  d_tab: 16 bytes of device memory.
template <size_t NBYTES, class T_CTX, class T_NEXT>
class THip11aSc : public HipFilter<T_CTX, T_NEXT> {
public:
    using iport_traits = port_traits<uint8_t, NBYTES>;
    using oport_traits = port_traits<uint8_t, NBYTES>;
    static constexpr uint32_t kNoTail = 0xFFFFFFFFu;
    THip11aSc(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* d_tab, uint8_t seed = 0xFF, void* stream = nullptr)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, stream), opin_(d_out), d_tab_(static_cast<uint32_t*>(d_tab)), seed_(seed), reg_(seed) {}
    void SetSeed(uint8_t seed) { seed_ = seed; }
    void SetTail(uint32_t byte_of_frame) { tail_ = byte_of_frame; }
    void Reset() { reg_ = seed_; done_ = 0; HipFilter<T_CTX, T_NEXT>::Reset(); }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            uint8_t* out = opin_.append();
            const uint32_t tail = (tail_ != kNoTail && tail_ >= done_ && tail_ - done_ < NBYTES) ? tail_ - done_ : kNoTail;
            const uint32_t tab[4] = { 0u, (uint32_t)NBYTES, tail, (uint32_t)reg_ };          // off, len, tail, seed (its low byte)
            if (sora_hip_memcpy_h2d(d_tab_, tab, sizeof(tab)) != SORA_OK) return this->raise(SORA_ERR_HARDWARE_FAILED);
            if (!this->raise(sora_hip_scramble11a(ipin.peek(), out, d_tab_, d_tab_ + 1, d_tab_ + 2, reinterpret_cast<const uint8_t*>(d_tab_ + 3), 1, NBYTES, this->stream_)))
                return false;
            for (size_t i = 0; i < NBYTES % 127 + 127; i++) reg_ = step(reg_);                 // (the 7-bit state has period 127 in byte steps)
            done_ += (uint32_t)NBYTES;
            ipin.pop();
            if (this->next_ && !this->next_->Process(opin_)) return false;
        }
        return true;
    }
    DevicePin<uint8_t, NBYTES>& opin() { return opin_; }
private:
    static uint8_t step(uint8_t reg)                                                           // m_Reg = m_lut[m_Reg >> 1] (scramble.hpp:192-201)
    {
        uint8_t x = (uint8_t)((reg >> 1) << 1);
        for (int k = 0; k < 8; k++) { const uint8_t o1 = ((x >> 1) ^ (x >> 4)) & 1; x = (uint8_t)((x >> 1) | (o1 << 7)); }
        return x;
    }
    DevicePin<uint8_t, NBYTES> opin_; uint32_t* d_tab_; uint8_t seed_, reg_; uint32_t tail_ = kNoTail, done_ = 0;
};

// TConvEncode_12 / _23 / _34 (conv_enc.hpp:18-330), CR = SORA_CR_12 / _23 / _34: IPORT uchar x NIN (whole bursts of 1 / 2 / 3 bytes) -> OPORT uchar x NIN (CR + 2) / (CR + 1).
// The stage starts every call from register 0; the adapter carries m_reg by encoding each burst behind the previous burst's last 1 / 2 / 3 bytes (zeros after Reset) and
// handing on what follows their output.  d_work: kWorkBytes of device memory, 16-byte aligned, the adapter's own (it holds the output pin's buffer).
template <int CR, size_t NIN, class T_CTX, class T_NEXT>
class THipConvEncode : public HipFilter<T_CTX, T_NEXT> {
    static constexpr size_t BIN = CR + 1, BOUT = CR + 2;
    static_assert(CR >= 0 && CR <= 2 && NIN % BIN == 0 && NIN >= BIN, "whole bursts of the brick");
public:
    static constexpr size_t NOUT = NIN / BIN * BOUT;
    static constexpr size_t kInAt = 16, kOutAt = 16 + (BIN + NIN + 15) / 16 * 16 + 16 - BOUT, kWorkBytes = kOutAt + BOUT + NOUT;
    using iport_traits = port_traits<uint8_t, NIN>;
    using oport_traits = port_traits<uint8_t, NOUT>;
    THipConvEncode(T_CTX& ctx, T_NEXT* next, uint8_t* d_work, void* stream = nullptr)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, stream), w_(d_work), opin_(d_work + kOutAt + BOUT) {}
    void Reset() { fresh_ = true; HipFilter<T_CTX, T_NEXT>::Reset(); }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            if (fresh_) {                                                                          // m_reg = 0, and the tables of the call: in_off, len, out_off
                const uint32_t tab[4] = { (uint32_t)kInAt, (uint32_t)(BIN + NIN), (uint32_t)kOutAt, 0u };   // (word 3: BIN <= 3 zero bytes of history)
                if (sora_hip_stream_synchronize(this->stream_) != SORA_OK || sora_hip_memcpy_h2d(w_, tab, sizeof(tab)) != SORA_OK ||
                    sora_hip_memcpy_h2d(w_ + kInAt, tab + 3, BIN) != SORA_OK) return this->raise(SORA_ERR_HARDWARE_FAILED);
                fresh_ = false;
            }
            const uint32_t* t = reinterpret_cast<const uint32_t*>(w_);
            opin_.append();
            if (sora_hip_memcpy_d2d(w_ + kInAt + BIN, ipin.peek(), NIN, this->stream_) != SORA_OK) return this->raise(SORA_ERR_HARDWARE_FAILED);
            if (!this->raise(sora_hip_conv_encode11a(w_, t, t + 1, CR, w_, t + 2, 1, BIN + NIN, this->stream_))) return false;
            if (sora_hip_memcpy_d2d(w_ + kInAt, w_ + kInAt + NIN, BIN, this->stream_) != SORA_OK) return this->raise(SORA_ERR_HARDWARE_FAILED);
            ipin.pop();
            if (this->next_ && !this->next_->Process(opin_)) return false;
        }
        return true;
    }
    DevicePin<uint8_t, NOUT>& opin() { return opin_; }
private:
    uint8_t* w_; DevicePin<uint8_t, NOUT> opin_; bool fresh_ = true;
};

// T11aInterleave{BPSK,QPSK,QAM16,QAM64} (interleave.hpp:16-114): IPORT uchar x 6 N_BPSC -> OPORT uchar x 6 N_BPSC, N symbols per burst
struct CallInterleave11a { int nb; size_t n; int operator()(const uint8_t* in, uint8_t* out, void* st) const { return sora_hip_interleave11a(in, out, nb, n, st); } };
template <int N_BPSC, size_t N, class T_CTX, class T_NEXT>
struct THip11aInterleave : THipStage<uint8_t, 6 * N_BPSC * N, uint8_t, 6 * N_BPSC * N, CallInterleave11a, T_CTX, T_NEXT> {
    THip11aInterleave(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* stream = nullptr)
        : THipStage<uint8_t, 6 * N_BPSC * N, uint8_t, 6 * N_BPSC * N, CallInterleave11a, T_CTX, T_NEXT>(ctx, next, d_out, CallInterleave11a{ N_BPSC, N }, stream) {}
};
// TMap11a{BPSK,QPSK,QAM16,QAM64}<MOD> (mapper11a.hpp:8-300): IPORT uchar x 6 N_BPSC -> OPORT COMPLEX16 x 48; mod = the brick's MOD (0: the 802.11a amplitude)
struct CallMap11a { int nb, mod; size_t n; int operator()(const uint8_t* in, sora_complex16* out, void* st) const { return sora_hip_map11a(in, out, nb, mod, n, st); } };
template <int N_BPSC, size_t N, class T_CTX, class T_NEXT>
struct THipMap11a : THipStage<uint8_t, 6 * N_BPSC * N, sora_complex16, 48 * N, CallMap11a, T_CTX, T_NEXT> {
    THipMap11a(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, int mod = 0, void* stream = nullptr)
        : THipStage<uint8_t, 6 * N_BPSC * N, sora_complex16, 48 * N, CallMap11a, T_CTX, T_NEXT>(ctx, next, d_out, CallMap11a{ N_BPSC, mod, N }, stream) {}
};

// T11aAddPilot<BPSK_MOD> (pilot.hpp:30-118): IPORT COMPLEX16 x 48 -> OPORT COMPLEX16 x 64, N symbols of ONE frame per burst.  m_PilotIndex is the count of symbols
// since Reset (the first takes PilotSgn[127], the SIGNAL symbol's); d_tab: 16 bytes of device memory for the call's frame table.
template <size_t N, class T_CTX, class T_NEXT>
class THip11aAddPilot : public HipFilter<T_CTX, T_NEXT> {
public:
    using iport_traits = port_traits<sora_complex16, 48 * N>;
    using oport_traits = port_traits<sora_complex16, 64 * N>;
    THip11aAddPilot(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* d_tab, int bpsk_mod = 0, void* stream = nullptr)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, stream), opin_(d_out), d_tab_(static_cast<uint32_t*>(d_tab)), mod_(bpsk_mod) {}
    void Reset() { pos_ = 0; HipFilter<T_CTX, T_NEXT>::Reset(); }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            sora_complex16* out = opin_.append();
            const uint32_t tab[4] = { 0u, (uint32_t)N, pos_, 0u };                                 // first, nsym, position of the burst's first symbol in its frame
            if (sora_hip_memcpy_h2d(d_tab_, tab, sizeof(tab)) != SORA_OK) return this->raise(SORA_ERR_HARDWARE_FAILED);
            if (!this->raise(sora_hip_add_pilot11a_from(ipin.peek(), out, d_tab_, d_tab_ + 1, d_tab_ + 2, 1, mod_, this->stream_))) return false;
            pos_ += (uint32_t)N;
            ipin.pop();
            if (this->next_ && !this->next_->Process(opin_)) return false;
        }
        return true;
    }
    DevicePin<sora_complex16, 64 * N>& opin() { return opin_; }
private:
    DevicePin<sora_complex16, 64 * N> opin_; uint32_t* d_tab_; int mod_; uint32_t pos_ = 0;
};

// TIFFTx (fft.hpp:7-61): IPORT COMPLEX16 x 64 -> OPORT COMPLEX16 x 160, N symbols per burst
struct CallIFFTx { size_t n; int operator()(const sora_complex16* in, sora_complex16* out, void* st) const { return sora_hip_ifftx11a(in, out, n, st); } };
template <size_t N, class T_CTX, class T_NEXT>
struct THipIFFTx : THipStage<sora_complex16, 64 * N, sora_complex16, 160 * N, CallIFFTx, T_CTX, T_NEXT> {
    THipIFFTx(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 64 * N, sora_complex16, 160 * N, CallIFFTx, T_CTX, T_NEXT>(ctx, next, d_out, CallIFFTx{ N }, stream) {}
};
// TUpsample40MTo44M (sampling.hpp:8-32): IPORT COMPLEX16 x 160 -> OPORT COMPLEX16 x 176, N blocks per burst.  d_sees_next: N device bytes, block b of a burst finds block
// b + 1's first sample behind its last one (the preamble source's one burst of four blocks: 1, 1, 1, 0); null: every block ends in x[160] = 0.
struct CallUpsample40to44 { const uint8_t* d_sees_next; size_t n; int operator()(const sora_complex16* in, sora_complex16* out, void* st) const
    { return sora_hip_upsample40to44(in, out, d_sees_next, n, st); } };
template <size_t N, class T_CTX, class T_NEXT>
struct THipUpsample40MTo44M : THipStage<sora_complex16, 160 * N, sora_complex16, 176 * N, CallUpsample40to44, T_CTX, T_NEXT> {
    THipUpsample40MTo44M(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, const uint8_t* d_sees_next = nullptr, void* stream = nullptr)
        : THipStage<sora_complex16, 160 * N, sora_complex16, 176 * N, CallUpsample40to44, T_CTX, T_NEXT>(ctx, next, d_out, CallUpsample40to44{ d_sees_next, N }, stream) {}
};
// TPackSample16to8 (stdbrick.hpp:415-445): IPORT COMPLEX16 x NSAMPLES -> OPORT COMPLEX8 x NSAMPLES (int8 re, int8 im), NSAMPLES a multiple of the brick's 8
struct sora_complex8 { int8_t re, im; };
struct CallPack16to8 { size_t n; int operator()(const sora_complex16* in, sora_complex8* out, void* st) const { return sora_hip_pack16to8(in, &out->re, n, st); } };
template <size_t NSAMPLES, class T_CTX, class T_NEXT>
struct THipPackSample16to8 : THipStage<sora_complex16, NSAMPLES, sora_complex8, NSAMPLES, CallPack16to8, T_CTX, T_NEXT> {
    static_assert(NSAMPLES % 8 == 0, "whole bursts of TPackSample16to8");
    THipPackSample16to8(T_CTX& ctx, T_NEXT* next, sora_complex8* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, NSAMPLES, sora_complex8, NSAMPLES, CallPack16to8, T_CTX, T_NEXT>(ctx, next, d_out, CallPack16to8{ NSAMPLES }, stream) {}
};

// ------------------------------------------------------------------------------------------------
// The bricks of the 802.11n 2x2 modulation graphs (kernel/bb/demod11/fb11nmod_config.hpp) beyond the 802.11a ones above (T11aSc, TConvEncode_*, the SIG graph's
// T11aInterleaveBPSK and T11aAddPilot<30339> are THip11aSc, THipConvEncode, THip11aInterleave<1> and THip11aAddPilot with bpsk_mod 30339).  One burst = N symbols;
// kRow11n = the bricks' N_b bytes per stream and symbol.
constexpr size_t kRow11n(int n_bpsc) { return (size_t)(52 * n_bpsc + 7) / 8; }

// TStreamParser{BPSK,QPSK,QAM16,QAM64}_12 (streamparser.hpp): IPORT uchar x 13 N_BPSC -> OPORTS 0 and 1 uchar x N_b, a demux: Next0 and Next1 take the two spatial streams
template <int N_BPSC, size_t N, class T_CTX, class T_NEXT0, class T_NEXT1>
class THipStreamParser {
public:
    using iport_traits = port_traits<uint8_t, 13 * N_BPSC * N>;
    using oport_traits = port_traits<uint8_t, kRow11n(N_BPSC) * N>;
    THipStreamParser(T_CTX& ctx, T_NEXT0* next0, T_NEXT1* next1, uint8_t* d_out0, uint8_t* d_out1, void* stream = nullptr)
        : ctx_(ctx), next0_(next0), next1_(next1), opin0_(d_out0), opin1_(d_out1), stream_(stream) {}
    void Reset() { if (next0_) next0_->Reset(); if (next1_) next1_->Reset(); }
    void Flush() { if (next0_) next0_->Flush(); if (next1_) next1_->Flush(); }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            uint8_t* out0 = opin0_.append(); uint8_t* out1 = opin1_.append();
            const int rc = sora_hip_stream_parse11n(ipin.peek(), out0, out1, N_BPSC, N, stream_);
            if (rc != SORA_OK) { ctx_.error_code = (uint32_t)rc; return false; }
            ipin.pop();
            if (next0_ && !next0_->Process(opin0_)) return false;
            if (next1_ && !next1_->Process(opin1_)) return false;
        }
        return true;
    }
    DevicePin<uint8_t, kRow11n(N_BPSC) * N>& opin0() { return opin0_; }
    DevicePin<uint8_t, kRow11n(N_BPSC) * N>& opin1() { return opin1_; }
private:
    T_CTX& ctx_; T_NEXT0* next0_; T_NEXT1* next1_; DevicePin<uint8_t, kRow11n(N_BPSC) * N> opin0_, opin1_; void* stream_;
};

// T11nInterleave{BPSK,QPSK,QAM16,QAM64}_S1 / _S2 (interleave.hpp:116-123), SPATIAL_STREAM 0 / 1: IPORT uchar x N_b -> OPORT uchar x N_b
struct CallInterleave11n { int nb, ss; size_t n; int operator()(const uint8_t* in, uint8_t* out, void* st) const
    { return sora_hip_interleave11n(in, out, nb, ss, n, st); } };
template <int N_BPSC, int SPATIAL_STREAM, size_t N, class T_CTX, class T_NEXT>
struct THip11nInterleave : THipStage<uint8_t, kRow11n(N_BPSC) * N, uint8_t, kRow11n(N_BPSC) * N, CallInterleave11n, T_CTX, T_NEXT> {
    THip11nInterleave(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* stream = nullptr)
        : THipStage<uint8_t, kRow11n(N_BPSC) * N, uint8_t, kRow11n(N_BPSC) * N, CallInterleave11n, T_CTX, T_NEXT>(ctx, next, d_out,
              CallInterleave11n{ N_BPSC, SPATIAL_STREAM, N }, stream) {}
};
// TMap11a*<MOD> behind them: IPORT uchar x N_b -> OPORT COMPLEX16 x 52; mod = the brick's MOD (0: 30339 / 21453 / 9594 / 4681).  The BPSK brick's pin carries 56 carriers
// per symbol, of which T11nAddPilot drops the last four: this adapter hands on the 52.
struct CallMap11n { int nb, mod; size_t n; int operator()(const uint8_t* in, sora_complex16* out, void* st) const { return sora_hip_map11n(in, out, nb, mod, n, st); } };
template <int N_BPSC, size_t N, class T_CTX, class T_NEXT>
struct THipMap11n : THipStage<uint8_t, kRow11n(N_BPSC) * N, sora_complex16, 52 * N, CallMap11n, T_CTX, T_NEXT> {
    THipMap11n(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, int mod = 0, void* stream = nullptr)
        : THipStage<uint8_t, kRow11n(N_BPSC) * N, sora_complex16, 52 * N, CallMap11n, T_CTX, T_NEXT>(ctx, next, d_out, CallMap11n{ N_BPSC, mod, N }, stream) {}
};
// TSigMap11n (mapper11n.hpp): IPORT uchar x 18 -> OPORT COMPLEX16 x 144, N frames per burst
struct CallSigMap11n { size_t n; int operator()(const uint8_t* in, sora_complex16* out, void* st) const { return sora_hip_sig_map11n(in, out, n, st); } };
template <size_t N, class T_CTX, class T_NEXT>
struct THipSigMap11n : THipStage<uint8_t, 18 * N, sora_complex16, 144 * N, CallSigMap11n, T_CTX, T_NEXT> {
    THipSigMap11n(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<uint8_t, 18 * N, sora_complex16, 144 * N, CallSigMap11n, T_CTX, T_NEXT>(ctx, next, d_out, CallSigMap11n{ N }, stream) {}
};

// T11nAddPilot<ISS> (pilot_11n.hpp:7-82): IPORT COMPLEX16 x 52 -> OPORT COMPLEX16 x 64, N symbols of ONE frame per burst.  pilot_index is the count of symbols since
// Reset, handed to the stage through d_pos0; d_tab: 16 bytes of device memory for the call's frame table.
template <int ISS, size_t N, class T_CTX, class T_NEXT>
class THip11nAddPilot : public HipFilter<T_CTX, T_NEXT> {
public:
    using iport_traits = port_traits<sora_complex16, 52 * N>;
    using oport_traits = port_traits<sora_complex16, 64 * N>;
    THip11nAddPilot(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* d_tab, void* stream = nullptr)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, stream), opin_(d_out), d_tab_(static_cast<uint32_t*>(d_tab)) {}
    void Reset() { pos_ = 0; HipFilter<T_CTX, T_NEXT>::Reset(); }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            sora_complex16* out = opin_.append();
            const uint32_t tab[4] = { 0u, (uint32_t)N, pos_, 0u };                                 // first, nsym, position of the burst's first symbol in its frame
            if (sora_hip_memcpy_h2d(d_tab_, tab, sizeof(tab)) != SORA_OK) return this->raise(SORA_ERR_HARDWARE_FAILED);
            if (!this->raise(sora_hip_add_pilot11n(ipin.peek(), out, d_tab_, d_tab_ + 1, d_tab_ + 2, 1, ISS, this->stream_))) return false;
            pos_ += (uint32_t)N;
            ipin.pop();
            if (this->next_ && !this->next_->Process(opin_)) return false;
        }
        return true;
    }
    DevicePin<sora_complex16, 64 * N>& opin() { return opin_; }
private:
    DevicePin<sora_complex16, 64 * N> opin_; uint32_t* d_tab_; uint32_t pos_ = 0;
};

// TIFFTxOnly (fft.hpp:63-103): IPORT COMPLEX16 x 64 -> OPORT COMPLEX16 x 128
struct CallIFFTxOnly { size_t n; int operator()(const sora_complex16* in, sora_complex16* out, void* st) const { return sora_hip_ifft_only11n(in, out, n, st); } };
template <size_t N, class T_CTX, class T_NEXT>
struct THipIFFTxOnly : THipStage<sora_complex16, 64 * N, sora_complex16, 128 * N, CallIFFTxOnly, T_CTX, T_NEXT> {
    THipIFFTxOnly(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 64 * N, sora_complex16, 128 * N, CallIFFTxOnly, T_CTX, T_NEXT>(ctx, next, d_out, CallIFFTxOnly{ N }, stream) {}
};
// TCSD<NCSD> (csd.hpp): IPORT COMPLEX16 x 128 -> OPORT COMPLEX16 x 128 (the output pin's buffer must not be the input pin's)
struct CallCSD { int ncsd; size_t n; int operator()(const sora_complex16* in, sora_complex16* out, void* st) const { return sora_hip_csd11n(in, out, ncsd, n, st); } };
template <int NCSD, size_t N, class T_CTX, class T_NEXT>
struct THipCSD : THipStage<sora_complex16, 128 * N, sora_complex16, 128 * N, CallCSD, T_CTX, T_NEXT> {
    static_assert(NCSD >= 1 && NCSD <= 31, "a delay of 4 .. 124 samples");
    THipCSD(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 128 * N, sora_complex16, 128 * N, CallCSD, T_CTX, T_NEXT>(ctx, next, d_out, CallCSD{ NCSD, N }, stream) {}
};
// TAddGI (gi.hpp): IPORT COMPLEX16 x 128 -> OPORT COMPLEX16 x 160
struct CallAddGI { size_t n; int operator()(const sora_complex16* in, sora_complex16* out, void* st) const { return sora_hip_add_gi11n(in, out, n, st); } };
template <size_t N, class T_CTX, class T_NEXT>
struct THipAddGI : THipStage<sora_complex16, 128 * N, sora_complex16, 160 * N, CallAddGI, T_CTX, T_NEXT> {
    THipAddGI(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 128 * N, sora_complex16, 160 * N, CallAddGI, T_CTX, T_NEXT>(ctx, next, d_out, CallAddGI{ N }, stream) {}
};

// ------------------------------------------------------------------------------------------------
// The fixed-ratio bricks of the 802.11b receive graph (kernel/bb/demod11/fb11bdemod_config.hpp:122-172), each where its SSE brick sits: one burst = N of the brick's own
// bursts, one stream per adapter.  What the bricks keep in context facades -- CF_DifferentialDemap::last_symbol, CF_Descramber::byte_reg -- lies in ONE device record
// (sora_stream11b_state) that the adapters of a graph share, as the bricks share their context: the demappers and the CCK decoders hand last_symbol on to each other, the
// descrambler keeps byte_reg there, and no Reset clears either; TCCK11Decoder's is_even is brick state in the same record and its Reset clears it.  The record carries
// the state from Process to Process by itself (the entry points read it and write it back).  d_tab: 16 bytes of device memory, the adapter's own (its stream table).
// The bricks that consume a variable number of items (TEnergyDetect, TSymTiming, TBarkerSync, TSFDSync) and the two sinks have entry points but no adapter.
template <class IT, size_t IB, class OT, size_t OB, class T_CTX, class T_NEXT>
class THip11bStage : public HipFilter<T_CTX, T_NEXT> {
public:
    using iport_traits = port_traits<IT, IB>;
    using oport_traits = port_traits<OT, OB>;
    THip11bStage(T_CTX& ctx, T_NEXT* next, OT* d_out, void* d_tab, uint32_t units, void* stream)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, stream), opin_(d_out), d_tab_(static_cast<uint32_t*>(d_tab)), units_(units) {}
    DevicePin<OT, OB>& opin() { return opin_; }
protected:
    // CALL: int(const IT* in, const uint32_t* d_first, const uint32_t* d_n, const uint32_t* d_out_first, const uint32_t* d_word3, OT* out, void* stream)
    template <class T_IPIN, class CALL> bool run(T_IPIN& ipin, CALL call)
    {
        while (ipin.check_read()) {
            if (dirty_) {                                                                          // first, n, out_first, one word of the brick's own
                const uint32_t tab[4] = { 0u, units_, 0u, word3_ };
                if (sora_hip_stream_synchronize(this->stream_) != SORA_OK || sora_hip_memcpy_h2d(d_tab_, tab, sizeof(tab)) != SORA_OK) return this->raise(SORA_ERR_HARDWARE_FAILED);
                dirty_ = false;
            }
            OT* out = opin_.append();
            if (!this->raise(call(ipin.peek(), d_tab_, d_tab_ + 1, d_tab_ + 2, d_tab_ + 3, out, this->stream_))) return false;
            ipin.pop();
            if (this->next_ && !this->next_->Process(opin_)) return false;
        }
        return true;
    }
    DevicePin<OT, OB> opin_; uint32_t* d_tab_; uint32_t units_, word3_ = 0; bool dirty_ = true;
};

// TDCRemove (dc.hpp:6-38): IPORT COMPLEX16 x 4 N -> OPORT COMPLEX16 x 4 N.  CF_VecDC = SetDC (what TDCEstimator, the host's or sora_hip_energy_detect11b's, last said).
template <size_t N, class T_CTX, class T_NEXT>
class THip11bDCRemove : public THip11bStage<sora_complex16, 4 * N, sora_complex16, 4 * N, T_CTX, T_NEXT> {
    using Base = THip11bStage<sora_complex16, 4 * N, sora_complex16, 4 * N, T_CTX, T_NEXT>;
public:
    THip11bDCRemove(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* d_tab, void* stream = nullptr) : Base(ctx, next, d_out, d_tab, (uint32_t)N, stream) {}
    void SetDC(sora_complex16 dc) { this->word3_ = (uint32_t)(uint16_t)dc.re | ((uint32_t)(uint16_t)dc.im << 16); this->dirty_ = true; }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        return this->run(ipin, [](const sora_complex16* in, const uint32_t* f, const uint32_t* n, const uint32_t* of, const uint32_t* dc, sora_complex16* out, void* st) {
            return sora_hip_dc_remove11b(in, f, n, of, reinterpret_cast<const sora_complex16*>(dc), out, 1, N, st); });
    }
};

// TBB11bDespread (barkerspread.hpp:277-303): IPORT COMPLEX16 x 11 N -> OPORT COMPLEX16 x N
template <size_t N, class T_CTX, class T_NEXT>
class THip11bDespread : public THip11bStage<sora_complex16, 11 * N, sora_complex16, N, T_CTX, T_NEXT> {
    using Base = THip11bStage<sora_complex16, 11 * N, sora_complex16, N, T_CTX, T_NEXT>;
public:
    THip11bDespread(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* d_tab, void* stream = nullptr) : Base(ctx, next, d_out, d_tab, (uint32_t)N, stream) {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        return this->run(ipin, [](const sora_complex16* in, const uint32_t* f, const uint32_t* n, const uint32_t* of, const uint32_t*, sora_complex16* out, void* st) {
            return sora_hip_despread11b(in, f, n, of, out, 1, N, st); });
    }
};

// The five bricks over the shared record: IPORT IT x UNIT N -> OPORT uchar x N through ENTRY (a sora_hip_*11b stream stage)
template <class IT, size_t UNIT, size_t N, int (*ENTRY)(const IT*, const uint32_t*, const uint32_t*, const uint32_t*, sora_stream11b_state*, uint8_t*, size_t, size_t, void*),
          class T_CTX, class T_NEXT>
class THip11bStreamStage : public THip11bStage<IT, UNIT * N, uint8_t, N, T_CTX, T_NEXT> {
    using Base = THip11bStage<IT, UNIT * N, uint8_t, N, T_CTX, T_NEXT>;
public:
    THip11bStreamStage(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* d_tab, sora_stream11b_state* d_state, void* stream = nullptr)
        : Base(ctx, next, d_out, d_tab, (uint32_t)N, stream), d_state_(d_state) {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        sora_stream11b_state* state = d_state_;
        return this->run(ipin, [state](const IT* in, const uint32_t* f, const uint32_t* n, const uint32_t* of, const uint32_t*, uint8_t* out, void* st) {
            return ENTRY(in, f, n, of, state, out, 1, N, st); });
    }
protected:
    sora_stream11b_state* d_state_;
};
// TDBPSKDemap (barkerspread.hpp:312-390), 8 -> 1; TDQPSKDemap (:396-454), 4 -> 1; TCCK5P5Decoder (cck.hpp:70-206), 16 -> 1; TDesc741 (scramble.hpp:93-170), 1 -> 1
template <size_t N, class T_CTX, class T_NEXT> using THip11bDBPSKDemap = THip11bStreamStage<sora_complex16, 8, N, sora_hip_dbpsk_demap11b, T_CTX, T_NEXT>;
template <size_t N, class T_CTX, class T_NEXT> using THip11bDQPSKDemap = THip11bStreamStage<sora_complex16, 4, N, sora_hip_dqpsk_demap11b, T_CTX, T_NEXT>;
template <size_t N, class T_CTX, class T_NEXT> using THip11bCCK5P5Decoder = THip11bStreamStage<sora_complex16, 16, N, sora_hip_cck5p5_decode11b, T_CTX, T_NEXT>;
template <size_t N, class T_CTX, class T_NEXT> using THip11bDesc741 = THip11bStreamStage<uint8_t, 1, N, sora_hip_desc741_11b, T_CTX, T_NEXT>;
// TCCK11Decoder (cck.hpp:255-763), 8 -> 1: Reset clears is_even (waiting for the stream: the record is the device's)
template <size_t N, class T_CTX, class T_NEXT>
class THip11bCCK11Decoder : public THip11bStreamStage<sora_complex16, 8, N, sora_hip_cck11_decode11b, T_CTX, T_NEXT> {
    using Base = THip11bStreamStage<sora_complex16, 8, N, sora_hip_cck11_decode11b, T_CTX, T_NEXT>;
public:
    using Base::Base;
    void Reset()
    {
        const uint32_t zero = 0;
        if (sora_hip_stream_synchronize(this->stream_) != SORA_OK || sora_hip_memcpy_h2d(&this->d_state_->is_even, &zero, sizeof(zero)) != SORA_OK)
            this->raise(SORA_ERR_HARDWARE_FAILED);
        HipFilter<T_CTX, T_NEXT>::Reset();
    }
};

// ------------------------------------------------------------------------------------------------
// The 40 MHz HT 2x2 receiver's stage bricks (sora_hip_*_ht40), one burst = N symbols (or one frame).  Where the reference's bricks of this
// kind have two ports (two RX chains in, two spatial streams out) the two are the two halves of one burst, as in THip11nMimoComp.  The stages that take device tables
// (data symbol, tracker) get a small device array d_tab, which the adapter fills once: one frame that owns the burst.  tests/cxx/rx_ht40_chain.cpp runs a frame through them.
//   THipHt40DataSymbol<N>   IPORT COMPLEX16 x 2 x 160 N -> OPORT COMPLEX16 x 2 x 128 N        (d_tab: 3 words)
struct CallDataSymbolHt40 {
    const uint32_t* d_tab; size_t n;
    int operator()(const sora_complex16* in, sora_complex16* out, void* st) const
    { return sora_hip_data_symbol_ht40(in, in + 160 * n, d_tab, d_tab + 1, d_tab + 2, out, out + 128 * n, 1, n, st); }
};
template <size_t N, class T_CTX, class T_NEXT>
struct THipHt40DataSymbol : THipStage<sora_complex16, 320 * N, sora_complex16, 256 * N, CallDataSymbolHt40, T_CTX, T_NEXT> {
    THipHt40DataSymbol(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, uint32_t* d_tab, void* stream = nullptr)
        : THipStage<sora_complex16, 320 * N, sora_complex16, 256 * N, CallDataSymbolHt40, T_CTX, T_NEXT>(ctx, next, d_out, CallDataSymbolHt40{ d_tab, N }, stream)
    { const uint32_t t[3] = { 0u, (uint32_t)N, 0u }; this->raise(sora_hip_memcpy_h2d(d_tab, t, sizeof(t))); }
};
//   THipHt40MimoEst         IPORT COMPLEX16 x 2 x 256 (HT-LTF 1 | 2 of chain 0, then of chain 1, after FFT<128>) -> OPORT COMPLEX16 x 512: the weights; d_noise_var: one
//                           float on the device or null (zero forcing); d_h: room for the channel matrix (512) or null
struct CallMimoEstHt40 {
    const float* d_noise_var; sora_complex16* d_h;
    int operator()(const sora_complex16* in, sora_complex16* out, void* st) const { return sora_hip_mimo_est_ht40(in, in + 256, d_noise_var, d_h, out, 1, st); }
};
template <class T_CTX, class T_NEXT>
struct THipHt40MimoEst : THipStage<sora_complex16, 512, sora_complex16, 512, CallMimoEstHt40, T_CTX, T_NEXT> {
    THipHt40MimoEst(T_CTX& ctx, T_NEXT* next, sora_complex16* d_w, const float* d_noise_var = nullptr, sora_complex16* d_h = nullptr, void* stream = nullptr)
        : THipStage<sora_complex16, 512, sora_complex16, 512, CallMimoEstHt40, T_CTX, T_NEXT>(ctx, next, d_w, CallMimoEstHt40{ d_noise_var, d_h }, stream) {}
};
//   THipHt40MimoComp<N>     IPORT COMPLEX16 x 2 x 128 N (chain 0 symbols, then chain 1) -> OPORT COMPLEX16 x 2 x 128 N (stream 0, then stream 1)
struct CallMimoCompHt40 {
    const sora_complex16* d_w; size_t n;
    int operator()(const sora_complex16* in, sora_complex16* out, void* st) const { return sora_hip_mimo_comp_ht40(d_w, nullptr, in, in + 128 * n, out, out + 128 * n, n, st); }
};
template <size_t N, class T_CTX, class T_NEXT>
struct THipHt40MimoComp : THipStage<sora_complex16, 256 * N, sora_complex16, 256 * N, CallMimoCompHt40, T_CTX, T_NEXT> {
    THipHt40MimoComp(T_CTX& ctx, T_NEXT* next, const sora_complex16* d_w, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 256 * N, sora_complex16, 256 * N, CallMimoCompHt40, T_CTX, T_NEXT>(ctx, next, d_out, CallMimoCompHt40{ d_w, N }, stream) {}
};
//   THipHt40PilotTrack<N>   IPORT COMPLEX16 x 2 x 128 N (stream 0 symbols, then stream 1) -> OPORT int16 x N: theta after each symbol; d_state: the frame's
//                           CF_FreqOffset_11n record (24 int16), read and written                  (d_tab: 2 words)
struct CallPilotTrackHt40 {
    int16_t* d_state; const uint32_t* d_tab; size_t n;
    int operator()(const sora_complex16* in, int16_t* out, void* st) const { return sora_hip_pilot_track_ht40(in, in + 128 * n, d_tab, d_tab + 1, d_state, out, 1, st); }
};
template <size_t N, class T_CTX, class T_NEXT>
struct THipHt40PilotTrack : THipStage<sora_complex16, 256 * N, int16_t, N, CallPilotTrackHt40, T_CTX, T_NEXT> {
    THipHt40PilotTrack(T_CTX& ctx, T_NEXT* next, int16_t* d_state, int16_t* d_theta, uint32_t* d_tab, void* stream = nullptr)
        : THipStage<sora_complex16, 256 * N, int16_t, N, CallPilotTrackHt40, T_CTX, T_NEXT>(ctx, next, d_theta, CallPilotTrackHt40{ d_state, d_tab, N }, stream)
    { const uint32_t t[2] = { 0u, (uint32_t)N }; this->raise(sora_hip_memcpy_h2d(d_tab, t, sizeof(t))); }
};
//   THipHt40Demap<N_BPSC, N>, THipHt40Deinterleave<N_BPSC, SPATIAL_STREAM, N>, THipHt40StreamJoin<N_BPSC, N> (stream 0's symbols, then stream 1's -> the joint job's bytes)
struct CallDemapHt40 { int nb; size_t n; int operator()(const sora_complex16* in, uint8_t* out, void* st) const { return sora_hip_demap_ht40(in, out, nb, n, st); } };
template <int N_BPSC, size_t N, class T_CTX, class T_NEXT>
struct THipHt40Demap : THipStage<sora_complex16, 128 * N, uint8_t, 108 * N_BPSC * N, CallDemapHt40, T_CTX, T_NEXT> {
    THipHt40Demap(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 128 * N, uint8_t, 108 * N_BPSC * N, CallDemapHt40, T_CTX, T_NEXT>(ctx, next, d_out, CallDemapHt40{ N_BPSC, N }, stream) {}
};
struct CallDeintHt40 { int nb, ss; size_t n; int operator()(const uint8_t* in, uint8_t* out, void* st) const { return sora_hip_deinterleave_ht40(in, out, nb, ss, n, st); } };
template <int N_BPSC, int SPATIAL_STREAM, size_t N, class T_CTX, class T_NEXT>
struct THipHt40Deinterleave : THipStage<uint8_t, 108 * N_BPSC * N, uint8_t, 108 * N_BPSC * N, CallDeintHt40, T_CTX, T_NEXT> {
    THipHt40Deinterleave(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* stream = nullptr)
        : THipStage<uint8_t, 108 * N_BPSC * N, uint8_t, 108 * N_BPSC * N, CallDeintHt40, T_CTX, T_NEXT>(ctx, next, d_out, CallDeintHt40{ N_BPSC, SPATIAL_STREAM, N }, stream) {}
};
struct CallStreamJoinHt40 { int nb; size_t n; int operator()(const uint8_t* in, uint8_t* out, void* st) const { return sora_hip_stream_join_ht40(in, in + 108 * nb * n, out, nb, n, st); } };
template <int N_BPSC, size_t N, class T_CTX, class T_NEXT>
struct THipHt40StreamJoin : THipStage<uint8_t, 216 * N_BPSC * N, uint8_t, 216 * N_BPSC * N, CallStreamJoinHt40, T_CTX, T_NEXT> {
    THipHt40StreamJoin(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* stream = nullptr)
        : THipStage<uint8_t, 216 * N_BPSC * N, uint8_t, 216 * N_BPSC * N, CallStreamJoinHt40, T_CTX, T_NEXT>(ctx, next, d_out, CallStreamJoinHt40{ N_BPSC, N }, stream) {}
};
//   THipHt40NoiseVar        IPORT COMPLEX16 x 2 x 128 (the two L-LTF symbols of chain 0, then of chain 1, after FFT<64>) -> OPORT float x 1; d_S: the integer sum or null
struct CallNoiseVarHt40 { uint64_t* d_S; int operator()(const sora_complex16* in, float* out, void* st) const { return sora_hip_noise_var_ht40(in, in + 128, d_S, out, 1, st); } };
template <class T_CTX, class T_NEXT>
struct THipHt40NoiseVar : THipStage<sora_complex16, 256, float, 1, CallNoiseVarHt40, T_CTX, T_NEXT> {
    THipHt40NoiseVar(T_CTX& ctx, T_NEXT* next, float* d_out, uint64_t* d_S = nullptr, void* stream = nullptr)
        : THipStage<sora_complex16, 256, float, 1, CallNoiseVarHt40, T_CTX, T_NEXT>(ctx, next, d_out, CallNoiseVarHt40{ d_S }, stream) {}
};
// (sora_hip_downsample_ht40 has no fixed ratio per call -- a stream's parity runs on from call to call -- and stays a plain entry point.)

// ------------------------------------------------------------------------------------------------
// The bricks of the 40 MHz HT 2x2 modulation graph (include/sora_hip.h: the sora_hip_*_ht40 stages behind sora_hip_tx_ht40) beyond the 802.11a ones above (the
// scrambler, the encoder and the SIG symbols' BPSK interleaver are THip11aSc, THipConvEncode and THip11aInterleave<1>).  One burst = N symbols; kRowHt40 = N_b40
// bytes per stream and symbol.  The preamble source (sora_hip_preamble_ht40) and the stream-form interleaver (sora_hip_interleave_ht40_stream: frame tables, bit
// addresses) have no fixed ratio per burst and stay plain entry points.
constexpr size_t kRowHt40(int n_bpsc) { return (size_t)(108 * n_bpsc + 7) / 8; }

// the stream parser: IPORT uchar x 27 N_BPSC -> OPORTS 0 and 1 uchar x N_b40, a demux: Next0 and Next1 take the two spatial streams
template <int N_BPSC, size_t N, class T_CTX, class T_NEXT0, class T_NEXT1>
class THipHt40StreamParser {
public:
    using iport_traits = port_traits<uint8_t, 27 * N_BPSC * N>;
    using oport_traits = port_traits<uint8_t, kRowHt40(N_BPSC) * N>;
    THipHt40StreamParser(T_CTX& ctx, T_NEXT0* next0, T_NEXT1* next1, uint8_t* d_out0, uint8_t* d_out1, void* stream = nullptr)
        : ctx_(ctx), next0_(next0), next1_(next1), opin0_(d_out0), opin1_(d_out1), stream_(stream) {}
    void Reset() { if (next0_) next0_->Reset(); if (next1_) next1_->Reset(); }
    void Flush() { if (next0_) next0_->Flush(); if (next1_) next1_->Flush(); }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            uint8_t* out0 = opin0_.append(); uint8_t* out1 = opin1_.append();
            const int rc = sora_hip_stream_parse_ht40(ipin.peek(), out0, out1, N_BPSC, N, stream_);
            if (rc != SORA_OK) { ctx_.error_code = (uint32_t)rc; return false; }
            ipin.pop();
            if (next0_ && !next0_->Process(opin0_)) return false;
            if (next1_ && !next1_->Process(opin1_)) return false;
        }
        return true;
    }
    DevicePin<uint8_t, kRowHt40(N_BPSC) * N>& opin0() { return opin0_; }
    DevicePin<uint8_t, kRowHt40(N_BPSC) * N>& opin1() { return opin1_; }
private:
    T_CTX& ctx_; T_NEXT0* next0_; T_NEXT1* next1_; DevicePin<uint8_t, kRowHt40(N_BPSC) * N> opin0_, opin1_; void* stream_;
};
// the HT interleaver for 40 MHz, SPATIAL_STREAM 0 / 1: IPORT uchar x N_b40 -> OPORT uchar x N_b40
struct CallInterleaveHt40 { int nb, ss; size_t n; int operator()(const uint8_t* in, uint8_t* out, void* st) const
    { return sora_hip_interleave_ht40(in, out, nb, ss, n, st); } };
template <int N_BPSC, int SPATIAL_STREAM, size_t N, class T_CTX, class T_NEXT>
struct THipHt40Interleave : THipStage<uint8_t, kRowHt40(N_BPSC) * N, uint8_t, kRowHt40(N_BPSC) * N, CallInterleaveHt40, T_CTX, T_NEXT> {
    THipHt40Interleave(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* stream = nullptr)
        : THipStage<uint8_t, kRowHt40(N_BPSC) * N, uint8_t, kRowHt40(N_BPSC) * N, CallInterleaveHt40, T_CTX, T_NEXT>(ctx, next, d_out,
              CallInterleaveHt40{ N_BPSC, SPATIAL_STREAM, N }, stream) {}
};
// the mapper: IPORT uchar x N_b40 -> OPORT COMPLEX16 x 108
struct CallMapHt40 { int nb; size_t n; int operator()(const uint8_t* in, sora_complex16* out, void* st) const { return sora_hip_map_ht40(in, out, nb, n, st); } };
template <int N_BPSC, size_t N, class T_CTX, class T_NEXT>
struct THipHt40Map : THipStage<uint8_t, kRowHt40(N_BPSC) * N, sora_complex16, 108 * N, CallMapHt40, T_CTX, T_NEXT> {
    THipHt40Map(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<uint8_t, kRowHt40(N_BPSC) * N, sora_complex16, 108 * N, CallMapHt40, T_CTX, T_NEXT>(ctx, next, d_out, CallMapHt40{ N_BPSC, N }, stream) {}
};
// L-SIG + HT-SIG: IPORT uchar x 18 -> OPORT COMPLEX16 x 3 x 128, N frames per burst
struct CallSigMapHt40 { size_t n; int operator()(const uint8_t* in, sora_complex16* out, void* st) const { return sora_hip_sig_map_ht40(in, out, n, st); } };
template <size_t N, class T_CTX, class T_NEXT>
struct THipHt40SigMap : THipStage<uint8_t, 18 * N, sora_complex16, 384 * N, CallSigMapHt40, T_CTX, T_NEXT> {
    THipHt40SigMap(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<uint8_t, 18 * N, sora_complex16, 384 * N, CallSigMapHt40, T_CTX, T_NEXT>(ctx, next, d_out, CallSigMapHt40{ N }, stream) {}
};
// data carriers and pilots onto the 128 bins: IPORT COMPLEX16 x 108 -> OPORT COMPLEX16 x 128; the pilots do not depend on the symbol's place in its frame, so every
// burst is one frame of N symbols.  d_tab: 16 bytes of device memory for the call's frame table.
struct CallAddPilotHt40 {
    uint32_t* d_tab; size_t n;
    int operator()(const sora_complex16* in, sora_complex16* out, void* st) const
    {
        const uint32_t tab[4] = { 0u, (uint32_t)n, 0u, 0u };                                       // first, nsym
        if (sora_hip_memcpy_h2d(d_tab, tab, sizeof(tab)) != SORA_OK) return SORA_ERR_HARDWARE_FAILED;
        return sora_hip_add_pilot_ht40(in, out, d_tab, d_tab + 1, 1, st);
    }
};
template <size_t N, class T_CTX, class T_NEXT>
struct THipHt40AddPilot : THipStage<sora_complex16, 108 * N, sora_complex16, 128 * N, CallAddPilotHt40, T_CTX, T_NEXT> {
    THipHt40AddPilot(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* d_tab, void* stream = nullptr)
        : THipStage<sora_complex16, 108 * N, sora_complex16, 128 * N, CallAddPilotHt40, T_CTX, T_NEXT>(ctx, next, d_out,
              CallAddPilotHt40{ static_cast<uint32_t*>(d_tab), N }, stream) {}
};
// the fixed-point IFFT<128>, natural order: IPORT COMPLEX16 x 128 -> OPORT COMPLEX16 x 128
struct CallIFFTHt40 { size_t n; int operator()(const sora_complex16* in, sora_complex16* out, void* st) const { return sora_hip_ifft_ht40(in, out, n, st); } };
template <size_t N, class T_CTX, class T_NEXT>
struct THipHt40IFFT : THipStage<sora_complex16, 128 * N, sora_complex16, 128 * N, CallIFFTHt40, T_CTX, T_NEXT> {
    THipHt40IFFT(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 128 * N, sora_complex16, 128 * N, CallIFFTHt40, T_CTX, T_NEXT>(ctx, next, d_out, CallIFFTHt40{ N }, stream) {}
};
// the guard interval, GI 0 (long) / 1 (short): IPORT COMPLEX16 x 128 -> OPORT COMPLEX16 x 160 / 144
struct CallAddGIHt40 { int gi; size_t n; int operator()(const sora_complex16* in, sora_complex16* out, void* st) const { return sora_hip_add_gi_ht40(in, out, gi, n, st); } };
template <int GI, size_t N, class T_CTX, class T_NEXT>
struct THipHt40AddGI : THipStage<sora_complex16, 128 * N, sora_complex16, (GI ? 144 : 160) * N, CallAddGIHt40, T_CTX, T_NEXT> {
    static_assert(GI == 0 || GI == 1, "0 = long, 1 = short");
    THipHt40AddGI(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* stream = nullptr)
        : THipStage<sora_complex16, 128 * N, sora_complex16, (GI ? 144 : 160) * N, CallAddGIHt40, T_CTX, T_NEXT>(ctx, next, d_out, CallAddGIHt40{ GI, N }, stream) {}
};


// ------------------------------------------------------------------------------------------------
// The bricks that complete the 802.11n receive graph (kernel/bb/demod11/fb11ndemod_config.hpp:166-264), each where its SSE brick sits.  The bricks with NSTREAM = 2 ports
// carry the two chains / spatial streams as the two halves of one burst, as THip11nMimoComp does.  d_tab: 16 bytes of device memory, the adapter's own (its tables).
// T11nDataSymbol (PHY_11n.hpp:288-356): IPORT COMPLEX16 x 2 x 80 N (chain 0's N symbols, then chain 1's) -> OPORT COMPLEX16 x 2 x 64 N.  remain_symbols and the Flush at
// zero stay the host's.
template <size_t N, class T_CTX, class T_NEXT>
class THip11nDataSymbol : public THip11bStage<sora_complex16, 160 * N, sora_complex16, 128 * N, T_CTX, T_NEXT> {
    using Base = THip11bStage<sora_complex16, 160 * N, sora_complex16, 128 * N, T_CTX, T_NEXT>;
public:
    THip11nDataSymbol(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* d_tab, void* stream = nullptr) : Base(ctx, next, d_out, d_tab, (uint32_t)N, stream) {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        return this->run(ipin, [](const sora_complex16* in, const uint32_t* f, const uint32_t* n, const uint32_t* of, const uint32_t*, sora_complex16* out, void* st) {
            return sora_hip_data_symbol11n(in, in + 80 * N, f, n, of, out, out + 64 * N, 1, N, st); });
    }
};
// TStreamJoin<2, 52 N_BPSC> -> TStreamConcat<2, max(N_BPSC / 2, 1)> (stdbrick.hpp:640-720): IPORT uchar x 2 x 52 N_BPSC N (stream 0's N symbols, then stream 1's) ->
// OPORT uchar x 104 N_BPSC N, the decoder's soft stream
struct CallStreamJoin11n { int nb; size_t n; int operator()(const uint8_t* in, uint8_t* out, void* st) const { return sora_hip_stream_join11n(in, in + 52 * nb * n, out, nb, n, st); } };
template <int N_BPSC, size_t N, class T_CTX, class T_NEXT>
struct THip11nStreamJoin : THipStage<uint8_t, 104 * N_BPSC * N, uint8_t, 104 * N_BPSC * N, CallStreamJoin11n, T_CTX, T_NEXT> {
    THip11nStreamJoin(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* stream = nullptr)
        : THipStage<uint8_t, 104 * N_BPSC * N, uint8_t, 104 * N_BPSC * N, CallStreamJoin11n, T_CTX, T_NEXT>(ctx, next, d_out, CallStreamJoin11n{ N_BPSC, N }, stream) {}
};
// T11aDesc (scramble.hpp:269-355), behind the trellis of the 802.11a graph as of the 802.11n one: IPORT uchar x frame_length + 2 (what the trellis stages write) -> OPORT
// uchar x frame_length.  Like the trellis adapter it knows the frame from the context (SetFrame = CF_11aRxVector::frame_length).
template <class T_CTX, class T_NEXT>
class THip11aDesc : public HipFilter<T_CTX, T_NEXT> {
public:
    THip11aDesc(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* d_tab, void* stream = nullptr)
        : HipFilter<T_CTX, T_NEXT>(ctx, next, stream), opin_(d_out), d_tab_(static_cast<uint32_t*>(d_tab)) {}
    void SetFrame(uint16_t frame_length) { len_ = frame_length; dirty_ = true; }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            if (dirty_) {                                                                          // off, len, out_off
                const uint32_t tab[4] = { 0u, len_, 0u, 0u };
                if (sora_hip_stream_synchronize(this->stream_) != SORA_OK || sora_hip_memcpy_h2d(d_tab_, tab, sizeof(tab)) != SORA_OK) return this->raise(SORA_ERR_HARDWARE_FAILED);
                dirty_ = false;
            }
            uint8_t* out = opin_.append();
            if (!this->raise(sora_hip_desc11a(ipin.peek(), d_tab_, d_tab_ + 1, out, d_tab_ + 2, 1, this->stream_))) return false;
            ipin.pop();
            if (this->next_ && !this->next_->Process(opin_)) return false;
        }
        return true;
    }
    DevicePin<uint8_t, 4096>& opin() { return opin_; }
private:
    DevicePin<uint8_t, 4096> opin_; uint32_t* d_tab_; uint32_t len_ = 0; bool dirty_ = true;
};
// The two sinks on context.  TBB11aFrameSink (PHY_11a.hpp:609-700): IPORT uchar x frame_length; fills CF_11aSink (CF_Error::error_code, CF_11aRxVector::crc32) and, as the
// brick does when it has decided, returns false.  d_rec: one sora_sink11a_rec of device memory.
struct CF_11aSink { uint32_t error_code = 0, frame_crc32 = 0; };
class THip11aFrameSink {
public:
    THip11aFrameSink(CF_11aSink& ctx, sora_sink11a_rec* d_rec, void* d_tab, void* stream = nullptr) : ctx_(ctx), d_rec_(d_rec), d_tab_(static_cast<uint32_t*>(d_tab)), stream_(stream) {}
    void SetFrame(uint16_t frame_length) { len_ = frame_length; }
    void Reset() {}
    void Flush() {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            const uint32_t tab[4] = { 0u, len_, 0u, 0u };
            sora_sink11a_rec rec;
            int rc = sora_hip_stream_synchronize(stream_);
            if (rc == SORA_OK) rc = sora_hip_memcpy_h2d(d_tab_, tab, sizeof(tab));
            if (rc == SORA_OK) rc = sora_hip_frame_sink11a(ipin.peek(), d_tab_, d_tab_ + 1, d_rec_, 1, stream_);
            if (rc == SORA_OK) rc = sora_hip_stream_synchronize(stream_);
            if (rc == SORA_OK) rc = sora_hip_memcpy_d2h(&rec, d_rec_, sizeof(rec));
            ipin.pop();
            if (rc != SORA_OK) { ctx_.error_code = (uint32_t)rc; return false; }
            ctx_.error_code = rec.error_code; ctx_.frame_crc32 = rec.frame_crc32;
            if (rec.error_code) return false;                                                      // E_ERROR_FRAME_OK / E_ERROR_CRC32_FAIL: the frame is over
        }
        return true;
    }
private:
    CF_11aSink& ctx_; sora_sink11a_rec* d_rec_; uint32_t* d_tab_; void* stream_; uint32_t len_ = 0;
};
// TCCA11n (cca_11n.hpp): IPORT COMPLEX16 x 2 x 4 N (chain 0's N bursts, then chain 1's), a sink: fills CF_11nCCA (CF_11CCA::cca_state, cca_pwr_reading, CF_Error::error_code)
// and reports the bursts it swallowed (used(): the rest of the burst queue is the frame's).  d_state: one sora_cca11n_state of device memory that the adapter constructs;
// Reset() is the brick's _reset() with the context cleared, as BB11nDemodCtx.Reset and RxThread's ResetCarrierSense do it.
struct CF_11nCCA { uint32_t cca_state = 0, cca_pwr_reading = 0, error_code = 0; };
template <size_t N>
class THip11nCCA {
public:
    THip11nCCA(CF_11nCCA& ctx, sora_cca11n_state* d_state, void* d_tab, unsigned flags = 0, void* stream = nullptr)
        : ctx_(ctx), d_state_(d_state), d_tab_(static_cast<uint32_t*>(d_tab)), flags_(flags), stream_(stream) {}
    void Flush() {}
    bool Reset()
    {
        const uint32_t zero[6] = { 0, 0, 0, 0, 0, 0 };                                             // cca_state, error_code | (cca_pwr_reading stands) | the three counters
        ctx_.cca_state = 0; ctx_.error_code = 0;
        return sora_hip_stream_synchronize(stream_) == SORA_OK && sora_hip_memcpy_h2d(d_state_, zero, 8) == SORA_OK &&
               sora_hip_memcpy_h2d(reinterpret_cast<uint32_t*>(d_state_) + 3, zero, 12) == SORA_OK;
    }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            int rc = SORA_OK;
            if (!constructed_) {
                sora_cca11n_state s{};
                for (auto& e : s.his_moving_energy) { e[0] = 0xFFFFFFFFu; e[1] = 0x7FFFFFFFu; }    // LLONG_MAX
                rc = sora_hip_memcpy_h2d(d_state_, &s, sizeof(s));
                constructed_ = rc == SORA_OK;
            }
            const uint32_t tab[4] = { 0u, (uint32_t)N, 0u, 0u };                                   // first, n, used
            uint32_t head[3] = { 0, 0, 0 };
            if (rc == SORA_OK) rc = sora_hip_stream_synchronize(stream_);
            if (rc == SORA_OK) rc = sora_hip_memcpy_h2d(d_tab_, tab, sizeof(tab));
            if (rc == SORA_OK) rc = sora_hip_cca11n(ipin.peek(), ipin.peek() + 4 * N, d_tab_, d_tab_ + 1, d_state_, d_tab_ + 2, 1, N, flags_, stream_);
            if (rc == SORA_OK) rc = sora_hip_stream_synchronize(stream_);
            if (rc == SORA_OK) rc = sora_hip_memcpy_d2h(head, d_state_, sizeof(head));
            if (rc == SORA_OK) rc = sora_hip_memcpy_d2h(&used_, d_tab_ + 2, sizeof(used_));
            ipin.pop();
            if (rc != SORA_OK) { ctx_.error_code = (uint32_t)rc; return false; }
            ctx_.cca_state = head[0]; ctx_.error_code = head[1]; ctx_.cca_pwr_reading = head[2];
        }
        return true;
    }
    uint32_t used() const { return used_; }
private:
    CF_11nCCA& ctx_; sora_cca11n_state* d_state_; uint32_t* d_tab_; unsigned flags_; void* stream_; uint32_t used_ = 0; bool constructed_ = false;
};

// ------------------------------------------------------------------------------------------------
// The front-end bricks of the 802.11a receive graph (kernel/bb/demod11/fb11ademod_config.hpp:169-232), each where its SSE brick sits: one burst = N of the brick's own
// bursts, one stream per adapter.  d_tab: 32 bytes of device memory, the adapter's own (its tables).
// TDCRemoveEx<4>::Filter (brick/inc/dc.hpp:46-86): IPORT COMPLEX16 x 4 N -> OPORT COMPLEX16 x 4 N.  CF_VecDC = SetDC (what THip11aDCEstimator, or the host's brick, last said).
template <size_t N, class T_CTX, class T_NEXT>
class THip11aDCRemoveEx : public THip11bStage<sora_complex16, 4 * N, sora_complex16, 4 * N, T_CTX, T_NEXT> {
    using Base = THip11bStage<sora_complex16, 4 * N, sora_complex16, 4 * N, T_CTX, T_NEXT>;
public:
    THip11aDCRemoveEx(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* d_tab, void* stream = nullptr) : Base(ctx, next, d_out, d_tab, (uint32_t)N, stream) {}
    void SetDC(sora_complex16 dc) { this->word3_ = (uint32_t)(uint16_t)dc.re | ((uint32_t)(uint16_t)dc.im << 16); this->dirty_ = true; }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        return this->run(ipin, [](const sora_complex16* in, const uint32_t* f, const uint32_t* n, const uint32_t* of, const uint32_t* dc, sora_complex16* out, void* st) {
            return sora_hip_dc_remove11a(in, f, n, of, reinterpret_cast<const sora_complex16*>(dc), out, 1, N, st); });
    }
};
// T11aDataSymbol (PHY_11a.hpp:361-430): IPORT COMPLEX16 x 80 N -> OPORT COMPLEX16 x 64 N.  remain_symbols and the Flush at zero stay the host's.
template <size_t N, class T_CTX, class T_NEXT>
class THip11aDataSymbol : public THip11bStage<sora_complex16, 80 * N, sora_complex16, 64 * N, T_CTX, T_NEXT> {
    using Base = THip11bStage<sora_complex16, 80 * N, sora_complex16, 64 * N, T_CTX, T_NEXT>;
public:
    THip11aDataSymbol(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* d_tab, void* stream = nullptr) : Base(ctx, next, d_out, d_tab, (uint32_t)N, stream) {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        return this->run(ipin, [](const sora_complex16* in, const uint32_t* f, const uint32_t* n, const uint32_t* of, const uint32_t*, sora_complex16* out, void* st) {
            return sora_hip_data_symbol11a(in, f, n, of, out, 1, N, st); });
    }
};
// T11aViterbiSig (viterbi.hpp:8-49): IPORT uchar x 48 N -> OPORT uint x N
struct CallViterbiSig11a { size_t n; int operator()(const uint8_t* in, uint32_t* out, void* st) const { return sora_hip_viterbi_sig11a(in, out, n, st); } };
template <size_t N, class T_CTX, class T_NEXT>
struct THip11aViterbiSig : THipStage<uint8_t, 48 * N, uint32_t, N, CallViterbiSig11a, T_CTX, T_NEXT> {
    THip11aViterbiSig(T_CTX& ctx, T_NEXT* next, uint32_t* d_out, void* stream = nullptr)
        : THipStage<uint8_t, 48 * N, uint32_t, N, CallViterbiSig11a, T_CTX, T_NEXT>(ctx, next, d_out, CallViterbiSig11a{ N }, stream) {}
};
// T11aPLCPParser (PHY_11a.hpp:518-604), a sink of uint x 1: fills CF_11aPLCP -- CF_11aRxVector's fields as the parser leaves them from 0 (partial behind a reject: see
// sora_hip_plcp_parse11a), remain_symbols = total_symbols, CF_11RxPLCPSwitch::plcp_state (1 = plcp_data) and CF_Error::error_code.  d_rec: one sora_plcp11a_rec.
struct CF_11aPLCP { uint32_t error_code = 0, data_rate_kbps = 0, frame_length = 0, code_rate = 0, total_symbols = 0, remain_symbols = 0, plcp_state = 0; };
class THip11aPLCPParser {
public:
    THip11aPLCPParser(CF_11aPLCP& ctx, sora_plcp11a_rec* d_rec, void* stream = nullptr) : ctx_(ctx), d_rec_(d_rec), stream_(stream) {}
    void Reset() {}
    void Flush() {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            sora_plcp11a_rec rec;
            int rc = sora_hip_plcp_parse11a(ipin.peek(), d_rec_, 1, stream_);
            if (rc == SORA_OK) rc = sora_hip_stream_synchronize(stream_);
            if (rc == SORA_OK) rc = sora_hip_memcpy_d2h(&rec, d_rec_, sizeof(rec));
            ipin.pop();
            if (rc != SORA_OK) { ctx_.error_code = (uint32_t)rc; return false; }
            ctx_.data_rate_kbps = rec.data_rate_kbps; ctx_.frame_length = rec.frame_length; ctx_.code_rate = rec.code_rate; ctx_.total_symbols = rec.total_symbols;
            if (rec.error_code) ctx_.error_code = rec.error_code;                                  // E_ERROR_PLCP_HEADER_FAIL; the brick's Process still returns true
            else { ctx_.remain_symbols = rec.total_symbols; ctx_.plcp_state = 1; }
        }
        return true;
    }
private:
    CF_11aPLCP& ctx_; sora_plcp11a_rec* d_rec_; void* stream_;
};
// TDCEstimator (dc.hpp:99-165): IPORT COMPLEX16 x 4 N, passed through untouched (not copied: hand the same pin on).  d_state: one sora_dcest11a_state that the
// adapter constructs (update_cnt 8); Reset() is the brick's __init (DC stands).  DC() = CF_VecDC::direct_current after the last burst (one element: the four are equal).
template <size_t N>
class THip11aDCEstimator {
public:
    THip11aDCEstimator(sora_dcest11a_state* d_state, void* d_tab, void* stream = nullptr) : d_state_(d_state), d_tab_(static_cast<uint32_t*>(d_tab)), stream_(stream) {}
    void Flush() {}
    bool Reset()
    {
        const uint32_t init[2] = { 8u, 0u };                                                       // update_cnt, sum_dc
        return sora_hip_stream_synchronize(stream_) == SORA_OK && sora_hip_memcpy_h2d(d_state_, init, sizeof(init)) == SORA_OK;
    }
    // n: the bursts of the pin's burst that count (THip11aCCA::npass() where the pin is its gated output)
    template <class T_IPIN> bool Process(T_IPIN& ipin, uint32_t n = (uint32_t)N)
    {
        while (ipin.check_read()) {
            int rc = SORA_OK;
            if (!constructed_) { const sora_dcest11a_state s = { 8u, { 0, 0 }, { 0, 0 }, 0u }; rc = sora_hip_memcpy_h2d(d_state_, &s, sizeof(s)); constructed_ = rc == SORA_OK; }
            const uint32_t tab[2] = { 0u, n };
            if (rc == SORA_OK) rc = sora_hip_stream_synchronize(stream_);
            if (rc == SORA_OK) rc = sora_hip_memcpy_h2d(d_tab_, tab, sizeof(tab));
            if (rc == SORA_OK) rc = sora_hip_dc_estimate11a(ipin.peek(), d_tab_, d_tab_ + 1, d_state_, 1, N, stream_);
            if (rc == SORA_OK) rc = sora_hip_stream_synchronize(stream_);
            if (rc == SORA_OK) rc = sora_hip_memcpy_d2h(&dc_, &d_state_->dc, sizeof(dc_));
            ipin.pop();
            if (rc != SORA_OK) return false;
        }
        return true;
    }
    sora_complex16 DC() const { return dc_; }
private:
    sora_dcest11a_state* d_state_; uint32_t* d_tab_; void* stream_; sora_complex16 dc_ = { 0, 0 }; bool constructed_ = false;
};
// TCCA11a (Brick11/src/cca.hpp:104-441): IPORT COMPLEX16 x 4 N (DC-removed), a sink with a gated output: fills CF_11aCCA (CF_11CCA's cca_state, cca_pwr_reading,
// cca_peak_index; cca_pwr_threshold is read when the record is constructed; CF_Error::error_code), reports the bursts it swallowed (used(): the rest of the burst is the
// frame's) and leaves the bursts it hands to TDCEstimator in opin() (npass() of them).  d_state: one sora_cca11a_state that the adapter constructs; Reset() is the brick's
// __init with cca_state and error_code cleared, as BB11aDemodContext::Reset and RxThread's ResetCarrierSense do it.
struct CF_11aCCA { uint32_t cca_state = 0, cca_pwr_threshold = 1000 * 1000, cca_pwr_reading = 0, cca_peak_index = 0, error_code = 0; };
template <size_t N>
class THip11aCCA {
public:
    THip11aCCA(CF_11aCCA& ctx, sora_cca11a_state* d_state, sora_complex16* d_gated, void* d_tab, unsigned flags = 0, void* stream = nullptr)
        : ctx_(ctx), d_state_(d_state), opin_(d_gated), d_tab_(static_cast<uint32_t*>(d_tab)), flags_(flags), stream_(stream) {}
    void Flush() {}
    bool Reset()
    {
        sora_cca11a_state s{};                                                                     // words 5 .. 43 are 0 after __init; words 2 .. 4 stand
        const uint32_t zero[2] = { 0, 0 };
        if (sora_hip_stream_synchronize(stream_) != SORA_OK || sora_hip_memcpy_h2d(d_state_, zero, 8) != SORA_OK ||
            sora_hip_memcpy_h2d(&d_state_->sync_state, &s.sync_state, sizeof(s) - 20) != SORA_OK) return false;
        ctx_.cca_state = 0; ctx_.error_code = 0;                                                   // only once the device record says so too
        return true;
    }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        while (ipin.check_read()) {
            int rc = SORA_OK;
            if (!constructed_) {
                sora_cca11a_state s{}; s.cca_pwr_threshold = ctx_.cca_pwr_threshold;
                rc = sora_hip_memcpy_h2d(d_state_, &s, sizeof(s));
                constructed_ = rc == SORA_OK;
            }
            const uint32_t tab[5] = { 0u, (uint32_t)N, 0u, 0u, 0u };                               // first, n, out_first, used, npass
            uint32_t head[5] = { 0, 0, 0, 0, 0 }, res[2] = { 0, 0 };
            if (rc == SORA_OK) rc = sora_hip_stream_synchronize(stream_);
            if (rc == SORA_OK) rc = sora_hip_memcpy_h2d(d_tab_, tab, sizeof(tab));
            if (rc == SORA_OK) rc = sora_hip_cca11a(ipin.peek(), d_tab_, d_tab_ + 1, d_tab_ + 2, d_state_, opin_.append(), d_tab_ + 3, d_tab_ + 4, 1, N, flags_, stream_);
            if (rc == SORA_OK) rc = sora_hip_stream_synchronize(stream_);
            if (rc == SORA_OK) rc = sora_hip_memcpy_d2h(head, d_state_, sizeof(head));
            if (rc == SORA_OK) rc = sora_hip_memcpy_d2h(res, d_tab_ + 3, sizeof(res));
            ipin.pop();
            if (rc != SORA_OK) { ctx_.error_code = (uint32_t)rc; return false; }
            ctx_.cca_state = head[0]; ctx_.error_code = head[1]; ctx_.cca_pwr_reading = head[3]; ctx_.cca_peak_index = head[4];
            used_ = res[0]; npass_ = res[1];
        }
        return true;
    }
    DevicePin<sora_complex16, 4 * N>& opin() { return opin_; }
    uint32_t used() const { return used_; }
    uint32_t npass() const { return npass_; }
private:
    CF_11aCCA& ctx_; sora_cca11a_state* d_state_; DevicePin<sora_complex16, 4 * N> opin_; uint32_t* d_tab_; unsigned flags_; void* stream_;
    uint32_t used_ = 0, npass_ = 0; bool constructed_ = false;
};

// ------------------------------------------------------------------------------------------------
// The bricks of the 802.11b modulation graph (kernel/bb/demod11/fb11bmod_config.hpp:28-50) behind TBB11bSrc (sora_hip_ppdu11b, or the host's) and TBB11bMRSelect (the
// host's: it only routes): one burst = N of the brick's own bursts, one stream per adapter, d_tab as above.  What the bricks keep lies in device records that the entry
// points read and write back, so the state crosses from Process to Process by itself: the four spreaders share ONE sora_mod11b_state as the bricks share
// CF_DifferentialMap::last_phase (no Reset clears it); TCCK11Encode's bEven is is_even of the same record and its Reset clears it; the scrambler has its register, which
// Reset sets to CF_ScramblerSeed::sc_seed; the shaper has its m_temps, which Reset clears.  Adapters of different burst sizes may share a record (the reference's pin
// queues re-burst between the bricks; here each burst size is an adapter of its own over the same state).
template <size_t N, class T_CTX, class T_NEXT>
class THip11bSc741 : public THip11bStage<uint8_t, N, uint8_t, N, T_CTX, T_NEXT> {            // TSc741 (scramble.hpp:7-88), 1 -> 1
    using Base = THip11bStage<uint8_t, N, uint8_t, N, T_CTX, T_NEXT>;
public:
    THip11bSc741(T_CTX& ctx, T_NEXT* next, uint8_t* d_out, void* d_tab, uint32_t* d_reg, uint8_t sc_seed = 0x6C, void* stream = nullptr)
        : Base(ctx, next, d_out, d_tab, (uint32_t)N, stream), d_reg_(d_reg), seed_(sc_seed) {}
    void SetSeed(uint8_t sc_seed) { seed_ = sc_seed; }                                        // 0x6C behind the long preamble, 0x1B behind the short one
    void Reset()
    {
        const uint32_t reg = seed_;
        if (sora_hip_stream_synchronize(this->stream_) != SORA_OK || sora_hip_memcpy_h2d(d_reg_, &reg, sizeof(reg)) != SORA_OK) this->raise(SORA_ERR_HARDWARE_FAILED);
        HipFilter<T_CTX, T_NEXT>::Reset();
    }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        uint32_t* reg = d_reg_;
        return this->run(ipin, [reg](const uint8_t* in, const uint32_t* f, const uint32_t* n, const uint32_t* of, const uint32_t*, uint8_t* out, void* st) {
            return sora_hip_sc741_11b(in, f, n, of, reg, out, 1, N, st); });
    }
private:
    uint32_t* d_reg_; uint8_t seed_;
};

// The four spreaders over the shared record: IPORT uchar x N -> OPORT COMPLEX8 x CHIPS N through ENTRY
template <size_t CHIPS, size_t N, int (*ENTRY)(const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, sora_mod11b_state*, int8_t*, size_t, size_t, void*),
          class T_CTX, class T_NEXT>
class THip11bSpreadStage : public THip11bStage<uint8_t, N, sora_complex8, CHIPS * N, T_CTX, T_NEXT> {
    using Base = THip11bStage<uint8_t, N, sora_complex8, CHIPS * N, T_CTX, T_NEXT>;
public:
    THip11bSpreadStage(T_CTX& ctx, T_NEXT* next, sora_complex8* d_out, void* d_tab, sora_mod11b_state* d_state, void* stream = nullptr)
        : Base(ctx, next, d_out, d_tab, (uint32_t)N, stream), d_state_(d_state) {}
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        sora_mod11b_state* state = d_state_;
        return this->run(ipin, [state](const uint8_t* in, const uint32_t* f, const uint32_t* n, const uint32_t* of, const uint32_t*, sora_complex8* out, void* st) {
            return ENTRY(in, f, n, of, state, &out->re, 1, N, st); });
    }
protected:
    sora_mod11b_state* d_state_;
};
// TBB11bDBPSKSpread (barkerspread.hpp:9-111), 1 -> 88; TBB11bDQPSKSpread (:113-225), 1 -> 44; TCCK5Encode (cck.hpp:880-953), 1 -> 16
template <size_t N, class T_CTX, class T_NEXT> using THip11bDBPSKSpread = THip11bSpreadStage<88, N, sora_hip_dbpsk_spread11b, T_CTX, T_NEXT>;
template <size_t N, class T_CTX, class T_NEXT> using THip11bDQPSKSpread = THip11bSpreadStage<44, N, sora_hip_dqpsk_spread11b, T_CTX, T_NEXT>;
template <size_t N, class T_CTX, class T_NEXT> using THip11bCCK5Encode = THip11bSpreadStage<16, N, sora_hip_cck5_encode11b, T_CTX, T_NEXT>;
// TCCK11Encode (cck.hpp:782-870), 1 -> 8: Reset clears bEven
template <size_t N, class T_CTX, class T_NEXT>
class THip11bCCK11Encode : public THip11bSpreadStage<8, N, sora_hip_cck11_encode11b, T_CTX, T_NEXT> {
    using Base = THip11bSpreadStage<8, N, sora_hip_cck11_encode11b, T_CTX, T_NEXT>;
public:
    using Base::Base;
    void Reset()
    {
        const uint32_t zero = 0;
        if (sora_hip_stream_synchronize(this->stream_) != SORA_OK || sora_hip_memcpy_h2d(&this->d_state_->is_even, &zero, sizeof(zero)) != SORA_OK)
            this->raise(SORA_ERR_HARDWARE_FAILED);
        HipFilter<T_CTX, T_NEXT>::Reset();
    }
};

// TQuickPulseShaper (pulse.hpp:254-384), 1 -> 4: IPORT COMPLEX8 x N -> OPORT COMPLEX16 x 4 N.  Flush runs the brick's five bursts from zero input (20 samples) and hands
// them on in whole output bursts, the last one padded with zeros as the reference's pin queue pads it for the brick behind: d_out has room for kFlushBursts bursts.
template <size_t N, class T_CTX, class T_NEXT>
class THip11bQuickPulseShaper : public THip11bStage<sora_complex8, N, sora_complex16, 4 * N, T_CTX, T_NEXT> {
    using Base = THip11bStage<sora_complex8, N, sora_complex16, 4 * N, T_CTX, T_NEXT>;
public:
    static constexpr size_t kFlushBursts = (20 + 4 * N - 1) / (4 * N);
    THip11bQuickPulseShaper(T_CTX& ctx, T_NEXT* next, sora_complex16* d_out, void* d_tab, sora_shaper11b_state* d_state, void* stream = nullptr)
        : Base(ctx, next, d_out, d_tab, (uint32_t)N, stream), d_state_(d_state) { this->word3_ = 1; }
    void Reset()
    {
        const sora_shaper11b_state zero{};
        if (sora_hip_stream_synchronize(this->stream_) != SORA_OK || sora_hip_memcpy_h2d(d_state_, &zero, sizeof(zero)) != SORA_OK) this->raise(SORA_ERR_HARDWARE_FAILED);
        HipFilter<T_CTX, T_NEXT>::Reset();
    }
    template <class T_IPIN> bool Process(T_IPIN& ipin)
    {
        sora_shaper11b_state* state = d_state_;
        return this->run(ipin, [state](const sora_complex8* in, const uint32_t* f, const uint32_t* n, const uint32_t* of, const uint32_t*, sora_complex16* out, void* st) {
            return sora_hip_pulse_shape11b(&in->re, f, n, of, nullptr, state, out, 1, N, st); });
    }
    void Flush()
    {
        const sora_complex16 zeros[kFlushBursts * 4 * N] = {};
        const uint32_t tab[4] = { 0u, (uint32_t)N, 0u, 1u };                                  // Process's table; its word 0 is the flush call's count, its word 3 the flag
        sora_complex16* out = this->opin_.append();
        this->opin_.clear();
        bool ok = sora_hip_stream_synchronize(this->stream_) == SORA_OK && sora_hip_memcpy_h2d(out, zeros, sizeof(zeros)) == SORA_OK &&
                  sora_hip_memcpy_h2d(this->d_tab_, tab, sizeof(tab)) == SORA_OK;
        if (!ok) this->raise(SORA_ERR_HARDWARE_FAILED);
        // no chips: d_in is not read, any device address serves
        ok = ok && this->raise(sora_hip_pulse_shape11b(reinterpret_cast<const int8_t*>(out), this->d_tab_, this->d_tab_, this->d_tab_ + 2,
                                                       reinterpret_cast<const uint8_t*>(this->d_tab_ + 3), d_state_, out, 1, 0, this->stream_));
        for (size_t k = 0; ok && this->next_ && k < kFlushBursts; k++) {
            DevicePin<sora_complex16, 4 * N> pin(out + k * 4 * N);
            pin.append();
            ok = this->next_->Process(pin);
        }
        HipFilter<T_CTX, T_NEXT>::Flush();
    }
private:
    sora_shaper11b_state* d_state_;
};

// ISource over a batch of captures = the whole demod graph behind one handle (brick.h:343-353: Process/Seek/Reset/Flush).
class THipRx11aSource {
public:
    THipRx11aSource(CF_Error& ctx, const sora_rx_cfg& cfg) : ctx_(ctx), rx_(nullptr) { ctx_.error_code = (uint32_t)sora_rx_create(&cfg, &rx_); }
    ~THipRx11aSource() { if (rx_) sora_rx_destroy(rx_); }
    THipRx11aSource(const THipRx11aSource&) = delete;
    THipRx11aSource& operator=(const THipRx11aSource&) = delete;
    void Bind(const sora_complex16* d_iq, const sora_capture_desc* caps, size_t ncaps) { d_iq_ = d_iq; caps_ = caps; ncaps_ = ncaps; }
    bool Process()
    {
        if (!rx_) return false;
        const int rc = sora_rx_process_dev(rx_, d_iq_, caps_, ncaps_);
        if (rc != SORA_OK) { ctx_.error_code = (uint32_t)rc; return false; }
        return true;
    }
    void Reset() { if (rx_) sora_rx_reset(rx_); }
    void Flush() { if (rx_) sora_rx_flush(rx_); }
    sora_rx_t* handle() { return rx_; }
private:
    CF_Error& ctx_; sora_rx_t* rx_;
    const sora_complex16* d_iq_ = nullptr; const sora_capture_desc* caps_ = nullptr; size_t ncaps_ = 0;
};

// The 802.11b graph as one ISource: CreateDemodGraph (fb11bdemod_config.hpp:122-172) + MAC11b_Receive over a batch of 44 MHz captures.
class THipRx11bSource {
public:
    THipRx11bSource(CF_Error& ctx, const sora_rx_cfg& cfg) : ctx_(ctx), rx_(nullptr) { ctx_.error_code = (uint32_t)sora_rx11b_create(&cfg, &rx_); }
    ~THipRx11bSource() { if (rx_) sora_rx11b_destroy(rx_); }
    THipRx11bSource(const THipRx11bSource&) = delete;
    THipRx11bSource& operator=(const THipRx11bSource&) = delete;
    void Bind(const sora_complex16* d_iq, const sora_capture_desc* caps, size_t ncaps) { d_iq_ = d_iq; caps_ = caps; ncaps_ = ncaps; }
    bool Process()
    {
        if (!rx_) return false;
        const int rc = sora_rx11b_process_dev(rx_, d_iq_, caps_, ncaps_);
        if (rc != SORA_OK) { ctx_.error_code = (uint32_t)rc; return false; }
        return true;
    }
    void Reset() {}                                      // every call starts from the graph's initial state
    void Flush() { if (rx_) (void)sora_rx11b_synchronize(rx_); }   // the handle keeps two calls in flight: Flush() = all of them have finished
    sora_rx11b_t* handle() { return rx_; }
private:
    CF_Error& ctx_; sora_rx11b_t* rx_;
    const sora_complex16* d_iq_ = nullptr; const sora_capture_desc* caps_ = nullptr; size_t ncaps_ = 0;
};

// The 802.11n 2x2 graph as one ISource: CreateDemodGraph11n (fb11ndemod_config.hpp:166-257) + RxThread over a batch of two-chain
// 40 MHz captures (what TMemSamples2 is initialised with: MemSamplesDesc::Init(2, InputBuf, nCnt), fb11n_demod.cpp:113-117).
class THipRx11nSource {
public:
    THipRx11nSource(CF_Error& ctx, const sora_rx_cfg& cfg) : ctx_(ctx), rx_(nullptr) { ctx_.error_code = (uint32_t)sora_rx11n_create(&cfg, &rx_); }
    ~THipRx11nSource() { if (rx_) sora_rx11n_destroy(rx_); }
    THipRx11nSource(const THipRx11nSource&) = delete;
    THipRx11nSource& operator=(const THipRx11nSource&) = delete;
    void Bind(const sora_complex16* d_iq0, const sora_complex16* d_iq1, const sora_capture_desc* caps, size_t ncaps) { d_iq_[0] = d_iq0; d_iq_[1] = d_iq1;
        caps_ = caps; ncaps_ = ncaps; }
    bool Process()
    {
        if (!rx_) return false;
        const int rc = sora_rx11n_process_dev(rx_, d_iq_[0], d_iq_[1], caps_, ncaps_);
        if (rc != SORA_OK) { ctx_.error_code = (uint32_t)rc; return false; }
        return true;
    }
    void Reset() {}                                      // every call starts from the graph's initial state
    void Flush() { if (rx_) (void)sora_rx11n_synchronize(rx_); }   // (sora_rx11n_set_depth calls in flight)
    sora_rx11n_t* handle() { return rx_; }
private:
    CF_Error& ctx_; sora_rx11n_t* rx_;
    const sora_complex16* d_iq_[2] = { nullptr, nullptr }; const sora_capture_desc* caps_ = nullptr; size_t ncaps_ = 0;
};

}  // namespace sora_brick
