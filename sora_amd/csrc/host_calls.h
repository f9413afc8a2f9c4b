// host_calls.h -- host side of the contract every receive handle (sora_rx, sora_rx11b, sora_rx11n, sora_ht40) keeps for its calls in flight (include/sora_hip.h):
// a call gets a ticket; a call whose delivery was enqueued (*_deliver_async) and that was waited for is RELEASED; the next call takes an unused slot, else the
// released call with the oldest ticket, else the oldest call; *_wait_any returns the oldest finished delivered call.  Also the stream-continuation records of
// the four handles and the checks the handles' entry points share.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <thread>
#include "../../include/sora_hip.h"

int sora_internal_fail(int code, const char* what, int hip_error);             // sora_hip.cpp: records the message sora_hip_last_error() returns
#define HIPCHK(call) do { hipError_t _e = (call); if (_e != hipSuccess) return sora_internal_fail(SORA_ERR_HARDWARE_FAILED, #call, (int)_e); } while (0)

namespace sora {

// "who: what" as the message sora_hip_last_error() returns -> code
inline int fail_at(int code, const std::string& who, const char* what, int hip_error = 0) { return sora_internal_fail(code, (who + ": " + what).c_str(), hip_error); }
inline int call_stale(const char* who)
{
    return fail_at(SORA_ERR_INVALID_PARAM, who, "stale ticket: its slot has been reused by a later process call (or the ticket was never issued)");
}

// One call in flight: the stream it runs on, its ticket (0: none) and how far it is.  A handle's slot / pipeline type derives from it.
struct Call {
    hipStream_t stream = nullptr;
    int ticket = 0;
    hipEvent_t ev_done = nullptr;             // recorded behind the last copy of the call's delivery
    bool delivered = false, released = false;
};

// A handle's calls are an array of n slots held by value (Slot s[n]) or of pipelines held by pointer (Pipe* s[n]; nullptr: not created yet).
template <typename C> inline C* call_ptr(C& c) { return &c; }
template <typename C> inline C* call_ptr(C* c) { return c; }

// the call that holds `ticket` among s[0, n), or nullptr
template <typename S> inline auto call_find(S* s, int n, int ticket) -> decltype(call_ptr(*s))
{
    if (ticket <= 0) return nullptr;
    for (int i = 0; i < n; i++) { const auto c = call_ptr(s[i]); if (c && c->ticket == ticket) return c; }
    return nullptr;
}

// The slot of the next call among s[0, n): an unused one (a pipeline not created yet counts as unused); else the released call with the oldest ticket (delivered
// and waited for: nothing of it is left to read on the device); else the oldest call -- plain rotation, the call then waits for that slot's stream.  A host that
// only ever waits for its oldest ticket sees a round-robin; one that takes completions as they come (*_wait_any) keeps every slot busy.
template <typename S> inline int call_next(S* s, int n)
{
    int best = -1, best_rel = -1;
    for (int i = 0; i < n; i++) {
        const auto c = call_ptr(s[i]);
        if (!c || c->ticket == 0) return i;
        if (c->released && (best_rel < 0 || c->ticket < call_ptr(s[best_rel])->ticket)) best_rel = i;
        if (best < 0 || c->ticket < call_ptr(s[best])->ticket) best = i;
    }
    return best_rel >= 0 ? best_rel : best;
}

// behind the last copy of a call's delivery
inline hipError_t call_mark_delivered(Call& c)
{
    if (!c.ev_done) { const hipError_t e = hipEventCreateWithFlags(&c.ev_done, hipEventDisableTiming); if (e != hipSuccess) return e; }
    const hipError_t e = hipEventRecord(c.ev_done, c.stream);
    if (e == hipSuccess) c.delivered = true;
    return e;
}

inline int call_wait(int device, Call& c)
{
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(c.stream));
    if (c.delivered) c.released = true;
    return SORA_OK;
}

// *ticket <- the finished delivered call with the oldest ticket among s[0, n), then wait(that ticket): the handle's *_wait, which releases it.  The ticket is
// reported even when that wait fails.  The calls' events are polled: no host thread blocks on the device meanwhile.  pre: the handle's prefix, for messages.
template <typename S, typename Wait> inline int calls_wait_any(S* s, int n, int device, int* ticket, const char* pre, Wait wait)
{
    *ticket = 0;
    HIPCHK(hipSetDevice(device));
    const std::string who = std::string(pre) + "_wait_any";
    for (unsigned spin = 0;; spin++) {
        decltype(call_ptr(*s)) done = nullptr; bool pending = false;
        for (int i = 0; i < n; i++) {
            const auto c = call_ptr(s[i]);
            if (!c || c->ticket == 0 || !c->delivered || c->released) continue;
            pending = true;
            const hipError_t q = hipEventQuery(c->ev_done);
            if (q == hipSuccess) { if (!done || c->ticket < done->ticket) done = c; }
            else if (q != hipErrorNotReady) { (void)hipGetLastError(); return fail_at(SORA_ERR_HARDWARE_FAILED, who, "hipEventQuery", (int)q); }
        }
        if (done) { *ticket = done->ticket; return wait(done->ticket); }
        if (!pending) return fail_at(SORA_ERR_FAILED, who, ("no call with an enqueued delivery (" + std::string(pre) + "_deliver_async) is in flight").c_str());
        (void)hipGetLastError();                                                    // (hipErrorNotReady is sticky for hipGetLastError)
        if (spin > 64) std::this_thread::yield();
    }
}

template <typename S> inline int calls_synchronize(S* s, int n, int device)
{
    HIPCHK(hipSetDevice(device));
    for (int i = 0; i < n; i++) { const auto c = call_ptr(s[i]); if (c) HIPCHK(hipStreamSynchronize(c->stream)); }
    return SORA_OK;
}

// Stream continuation (sora_rx_set_stream_mode and its 11b / 11n / HT40 twins): capture k of a call continues capture k of the call before it.  The handle owns, per
// capture, a continuation record of `words` words and a resume point.  Each handle serialises its calls in stream mode its own way.
struct StreamRecords {
    uint32_t words;                           // per capture: kContWords, kRec11bWords, kRec11nWords
    bool on = false;
    uint32_t* d_cont = nullptr; uint32_t* d_consumed = nullptr;     // allocated when the mode is first enabled

    int zero(uint32_t max_captures)           // every stream starts afresh
    {
        if (!d_cont) return SORA_OK;
        HIPCHK(hipMemset(d_cont, 0, 4 * (size_t)words * max_captures));
        HIPCHK(hipMemset(d_consumed, 0, 4 * (size_t)max_captures));
        return SORA_OK;
    }
    // -> the previous mode (enable < 0: only that).  The handle's calls have finished.
    int set(int enable, int device, uint32_t max_captures)
    {
        const int old = on ? 1 : 0;
        if (enable < 0) return old;
        HIPCHK(hipSetDevice(device));
        if (enable && !d_cont) {
            HIPCHK(hipMalloc((void**)&d_cont, 4 * (size_t)words * max_captures));
            HIPCHK(hipMalloc((void**)&d_consumed, 4 * (size_t)max_captures));
        }
        { const int rc = zero(max_captures); if (rc) return rc; }                  // switching either way starts every stream afresh
        on = enable != 0;
        return old;
    }
    void free() { (void)hipFree(d_cont); (void)hipFree(d_consumed); d_cont = d_consumed = nullptr; }
    // *_stream_consumed: the resume points of the first ncaps captures of call c (the one its ticket names; latest: it is the handle's most recent call)
    template <typename C> int consumed(const char* who, int device, const C* c, bool latest, uint32_t* h_consumed, size_t ncaps) const
    {
        if (!on) return fail_at(SORA_ERR_FAILED, who, "the handle is not in stream mode");
        if (!c || !latest) return fail_at(SORA_ERR_INVALID_PARAM, who, "only the most recent call's resume points exist");
        if (ncaps > c->ncaps) return fail_at(SORA_ERR_INVALID_PARAM, who, "more captures than the call had");
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (ncaps) HIPCHK(hipMemcpy(h_consumed, d_consumed, 4 * ncaps, hipMemcpyDeviceToHost));
        return SORA_OK;
    }
    // *_stream_record_of: a copy of capture `capture`'s continuation record as call c (its ticket's; latest: the handle's most recent call) left it
    template <typename C> int record_of(const char* who, int device, const C* c, bool latest, uint32_t capture, uint32_t* out, size_t cap_words, size_t* n_words) const
    {
        *n_words = 0;
        if (!on) return fail_at(SORA_ERR_INVALID_PARAM, who, "the handle is not in stream mode");
        if (!c || !latest) return fail_at(SORA_ERR_INVALID_PARAM, who, "only the most recent call's records exist");
        if (capture >= c->ncaps) return fail_at(SORA_ERR_INVALID_PARAM, who, "no such capture in this call");
        *n_words = words;
        if (cap_words < words) return fail_at(SORA_ERR_CAPACITY, who, "output buffer too small");
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(out, d_cont + (size_t)capture * words, 4 * (size_t)words, hipMemcpyDeviceToHost));
        return SORA_OK;
    }
};

// *_create of a handle configured by a sora_rx_cfg whose graph takes rate_mhz samples: the checks, then the device is current
inline int check_rx_cfg(const sora_rx_cfg* cfg, const void* out, uint32_t rate_mhz, const char* who)
{
    if (!cfg || !out || cfg->struct_size != sizeof(sora_rx_cfg)) return fail_at(SORA_ERR_INVALID_PARAM, who, "bad cfg");
    if (cfg->sample_rate_mhz != rate_mhz) return fail_at(SORA_ERR_INVALID_PARAM, who, ("the graph takes sample_rate_mhz = " + std::to_string(rate_mhz)).c_str());
    if (cfg->max_captures == 0 || cfg->max_total_samples == 0 || cfg->max_frames_per_capture == 0) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "zero capacity", 0);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return sora_internal_fail(SORA_ERR_NO_DEVICE, "no HIP device: this library has no CPU path", 0);
    if (cfg->device < 0 || cfg->device >= ndev) return sora_internal_fail(SORA_ERR_INVALID_PARAM, "device ordinal out of range", 0);
    HIPCHK(hipSetDevice(cfg->device));
    return SORA_OK;
}

// *_process (host samples): the buffer's size is known there, so no capture descriptor may reach past it
inline int check_caps_in_buffer(const sora_capture_desc* caps, size_t ncaps, size_t nsamples)
{
    for (size_t i = 0; caps && i < ncaps; i++)
        if (caps[i].offset > nsamples || caps[i].nsamples > nsamples - caps[i].offset) return sora_internal_fail(SORA_ERR_INVALID_PARAM,
                "a capture descriptor reaches past the end of the sample buffer", 0);
    return SORA_OK;
}

}  // namespace sora
