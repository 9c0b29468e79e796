// host_api.h — the host side of the C-ABI layer, for every translation unit that implements entry points: the context,
// HIP_TRY, the helpers gnsship_abi.hip defines, the growable device buffer, what every handle's create / run / destroy
// is made of (reject, launched, stage, copy_out, alloc_all, free_all, quiesce) and the high-dynamics correlator's plan.
// Nothing here is seen by a kernel.
#pragma once
#include <algorithm>
#include <cstdio>
#include <initializer_list>

#include "engine.h"

namespace gnsship {

// A device buffer that grows when a call needs more than it holds (reserve) and is freed with its handle (release).
// `dev` and `cap` always match: both empty, or `cap` bytes at `dev`.
struct DevBuf {
    void* dev = nullptr;
    size_t cap = 0;  // bytes
    template <class T>
    T* as() const
    {
        return static_cast<T*>(dev);
    }
};

}  // namespace gnsship

struct gnsship_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t events[16] = {};
    std::string last_error;
    // code bank
    std::vector<gnsship::CodeDesc> codes_host;  // ptr = device pointer
    gnsship::DevBuf codes_dev;                  // CodeDesc table
    bool codes_dirty = false;
    uint64_t codes_version = 0;  // bumped by every gnsship_code_set (holders of code pointers re-attach)
};

// last_error = "<the expression>: <HIP's text>"
#define HIP_TRY(ctx, expr)                                                \
    do {                                                                  \
        hipError_t _e = (expr);                                           \
        if (_e != hipSuccess) return gnsship::hip_fail((ctx), _e, #expr); \
    } while (0)

namespace gnsship {

int fail(gnsship_ctx* ctx, int code, const char* what);           // last_error = what (copied); returns code
int hip_fail(gnsship_ctx* ctx, hipError_t e, const char* where);  // last_error = "where: <HIP's text>"; E_NOMEM or E_DEVICE
int set_device(gnsship_ctx* ctx);
int sync_code_table(gnsship_ctx* ctx);  // upload the code bank's table when codes changed
size_t fmt_bytes(int fmt);              // bytes per sample of a GNSSHIP_FMT_C*, 0 for any other value
int chunks_per_item_setting();

// At least `bytes` bytes in `b`.  Enough already: no HIP call.  Otherwise wait for the stream (earlier launches may
// still read the old buffer), free the old buffer, allocate — stopping at the first error, which is reported as
// "<who>(<what>): <HIP's text>" and leaves `b` empty, never a pointer or a capacity the other does not match.
// *grew (when given): the buffer is a new allocation whose content is undefined.
static inline int reserve(gnsship_ctx* ctx, DevBuf& b, size_t bytes, const char* who, const char* what, bool* grew = nullptr)
{
    if (grew) *grew = false;
    if (b.cap >= bytes) return GNSSHIP_OK;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (b.dev && e == hipSuccess) e = hipFree(b.dev);
    b = DevBuf{};
    if (e == hipSuccess) e = hipMalloc(&b.dev, bytes);
    if (e != hipSuccess) {
        b.dev = nullptr;
        char where[128];
        std::snprintf(where, sizeof(where), "%s(%s)", who, what);
        return hip_fail(ctx, e, where);
    }
    b.cap = bytes;
    if (grew) *grew = true;
    return GNSSHIP_OK;
}

// for destroy functions, after the stream was waited for
static inline void release(DevBuf& b)
{
    if (b.dev) (void)hipFree(b.dev);
    b = DevBuf{};
}

// The pieces of an entry point.  `who` is its name ("gnsship_cond_run"): a rejection's text is "<who>: <what>"; `where`
// is passed to hip_fail as it stands ("gnsship_cond_run(launch)").  These texts are part of the C ABI
// (tests/test_gpu_stream_rejections.py, tests/test_gpu_tlm_rejections.py).  Order in every run call: argument checks,
// then set_device, then staging, then the launch.
static inline int reject(gnsship_ctx* ctx, int code, const char* who, const char* what)
{
    char buf[256];
    std::snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return fail(ctx, code, buf);
}

// after a kernel launch
static inline int launched(gnsship_ctx* ctx, const char* where)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GNSSHIP_OK : hip_fail(ctx, e, where);
}

// Host data of `bytes` bytes to a staging buffer that grows only when it is too small (a failure there is
// "<who>(<what>)"), then the copy on the stream (a failure there is "<who>(upload)").  `room`, where given, is the size
// a buffer that has to grow is given (a handle that sizes its stage once, to its largest run).
static inline int stage(gnsship_ctx* ctx, DevBuf& s, const void* host, size_t bytes, const char* who, const char* what, size_t room = 0)
{
    if (int rc = reserve(ctx, s, s.cap < bytes ? std::max(room, bytes) : bytes, who, what)) return rc;
    const hipError_t e = hipMemcpyAsync(s.dev, host, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) return GNSSHIP_OK;
    char up[128];
    std::snprintf(up, sizeof(up), "%s(upload)", who);
    return hip_fail(ctx, e, up);
}

// Copy what the caller asked for: the entries with a host pointer and a size, in order, then one stream synchronise —
// none when nothing was copied (a run without a host copy stays asynchronous).  Stops at the first failure.
struct DevCopy {
    void* host;
    const void* dev;
    size_t bytes;
};
static inline int copy_out(gnsship_ctx* ctx, const DevCopy* list, size_t count, const char* where)
{
    bool any = false;
    for (size_t i = 0; i < count; i++) {
        const DevCopy& c = list[i];
        if (!c.host || c.bytes == 0) continue;
        const hipError_t e = hipMemcpyAsync(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, where);
        any = true;
    }
    if (!any) return GNSSHIP_OK;
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    return e == hipSuccess ? GNSSHIP_OK : hip_fail(ctx, e, where);
}
static inline int copy_out(gnsship_ctx* ctx, std::initializer_list<DevCopy> list, const char* where)
{
    return copy_out(ctx, list.begin(), list.size(), where);
}

// A handle's fixed device buffers: `count` elements at *ptr, zeroed on the stream where `zero`.
struct DevAlloc {
    void** ptr;
    size_t bytes;
    bool zero;
};
template <class T>
static inline DevAlloc dev_alloc(T** ptr, size_t count, bool zero = false)
{
    return {reinterpret_cast<void**>(ptr), sizeof(T) * count, zero};
}
// every hipMalloc, then every hipMemsetAsync; stops at the first error (the caller destroys the handle, which frees)
static inline hipError_t alloc_all(gnsship_ctx* ctx, std::initializer_list<DevAlloc> list)
{
    hipError_t e = hipSuccess;
    for (const DevAlloc& b : list)
        if (e == hipSuccess) e = hipMalloc(b.ptr, b.bytes);
    for (const DevAlloc& b : list)
        if (e == hipSuccess && b.zero) e = hipMemsetAsync(*b.ptr, 0, b.bytes, ctx->stream);
    return e;
}
// what a destroy function opens with: nothing on the stream still reads the handle's buffers
static inline void quiesce(gnsship_ctx* ctx)
{
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
}
static inline void free_all(std::initializer_list<void*> owned)
{
    for (void* p : owned)
        if (p) (void)hipFree(p);
}

// Host-side plan of the high-dynamics jobs of a batch (or of one gnsship_corr_run): corr_hd_kernel.hip.
struct HdPlan {
    std::vector<HdJob> jobs;
    std::vector<HdChunk> chunks;
    int64_t n_anchors = 0;
    int max_code_len = 1;
    DevBuf jobs_dev, chunks_dev, anchors_dev, partials_dev;  // HdJob, HdChunk, HdAnchor, float[chunk][2·kMaxTaps]
};
// Derive one HdJob from a reference-style call; false when the arguments are outside what the
// reference itself can run (taps, shifts that would make its memcpy lengths negative).
bool derive_hd_job(const gnsship_corr_job& in, const float* code_dev, int code_len, int out_index, HdJob& out);
// Chunks + anchor layout for plan.jobs; grows and uploads the device copies for entry point `who`.
int hd_plan_upload(gnsship_ctx* ctx, HdPlan& plan, const char* who);
void hd_plan_free(HdPlan& plan);
// Doppler-chain anchors, per-chunk correlation, per-job reduction into out[out_index].
hipError_t launch_corr_hd(const void* samples, int fmt, const HdPlan& plan, float* out, hipStream_t stream);

}  // namespace gnsship
