// dev_buf_check.cpp — the contract of gnsship::reserve / release and of the helpers every handle's create, run and
// destroy are made of (stage, copy_out, alloc_all, free_all, quiesce, reject, launched; csrc/host_api.h) against a fake
// HIP runtime.
//
// Built without the HIP runtime: hipStreamSynchronize, hipFree, hipMalloc, hipMemcpyAsync, hipMemsetAsync, hipSetDevice,
// hipGetLastError, fail and hip_fail are defined here.  The fakes log every call, hand out real host blocks (so the
// address sanitizer sees a double free or a leak of the fake's own), keep the set of live allocations, really copy and
// clear (so the sanitizer sees a copy past either block), and fail the call whose name is in `fail_on` (a name with a
// count, "h2d#2", fails the second such call).
//
// Checked (tests/test_dev_buf.py runs this under -fsanitize=address,undefined):
//  * enough capacity: no HIP call, not "grew";
//  * a grow: synchronise, free (only when there is an old buffer), allocate, in that order; "grew"; cap = the request;
//  * an injected failure of each of the three steps: the buffer is {nullptr, 0}, nothing after the failed step ran,
//    hip_fail got "<who>(<what>)" and the code it returned is reserve's, not "grew", nothing is freed twice.  A failed
//    allocation leaves no live block.  A failed synchronise or free stops before the old block could be released: that
//    block — and only that — stays live (the stream or the allocator is in error; the handle's destroy would not do better);
//  * a reserve after each failure allocates afresh without a free;
//  * release frees once, empties the buffer, and is a no-op on an empty one;
//  * stage: reserve (to `room` where a buffer has to grow and room is given), then one host-to-device copy on the context's stream; a reserve failure reads "<who>(<what>)" and
//    copies nothing, a copy failure reads "<who>(upload)"; a buffer that is large enough sees the copy and no other call;
//  * copy_out: the entries with a host pointer and a size, in order, then exactly one synchronise; it stops at the first
//    failed copy without a synchronise; no call at all when every entry is null or empty; every failure reads `where`;
//  * alloc_all: every allocation before any memset, memsets only where asked and over the whole block; it stops at the
//    first failed allocation (no memset) or memset;
//  * free_all skips null entries and frees each of the others once; quiesce sets the device, then synchronises;
//  * reject forms "<who>: <what>" and returns the code; launched reports hipGetLastError under `where`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "host_api.h"

namespace {
std::vector<std::string> calls;
std::set<void*> live;
std::string fail_on, last_where, last_fail;
hipError_t last_error = hipSuccess;  // what hipGetLastError returns
int counted_calls = 0;               // calls seen of the name a "name#k" in fail_on counts
int frees_of_dead = 0;
const hipStream_t kStream = reinterpret_cast<hipStream_t>(0x5eed);
int failures = 0;

void expect(bool ok, const char* what, int line)
{
    if (ok) return;
    std::printf("FAIL line %d: %s\n", line, what);
    failures++;
}
#define EXPECT(c) expect((c), #c, __LINE__)

std::string log()
{
    std::string s;
    for (const auto& c : calls) s += c + " ";
    calls.clear();
    return s;
}
}  // namespace

namespace {
// true when this call (logged under `name`) is the one `fail_on` asks to fail: "name", or "name#k" for the k-th
bool injected(const std::string& name)
{
    if (fail_on.rfind(name + "#", 0) != 0) return fail_on == name;
    return ++counted_calls == std::atoi(fail_on.c_str() + name.size() + 1);
}
// every case sets the failure through this: the count of a "name#k" starts afresh
void fail_at(const std::string& what)
{
    fail_on = what;
    counted_calls = 0;
}
const char* on(hipStream_t s) { return s == kStream ? "" : "(other stream)"; }
}  // namespace

extern "C" hipError_t hipSetDevice(int device)
{
    calls.push_back("device:" + std::to_string(device));
    return hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) { return last_error; }
extern "C" hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s)
{
    const std::string name = kind == hipMemcpyHostToDevice ? "h2d" : kind == hipMemcpyDeviceToHost ? "d2h" : "copy(other kind)";
    calls.push_back(name + ":" + std::to_string(bytes) + on(s));
    if (injected(name)) return hipErrorInvalidValue;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
extern "C" hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s)
{
    calls.push_back("memset:" + std::to_string(bytes) + on(s));
    if (injected("memset")) return hipErrorInvalidValue;
    std::memset(dst, value, bytes);
    return hipSuccess;
}
extern "C" hipError_t hipStreamSynchronize(hipStream_t s)
{
    calls.push_back(s == kStream ? "sync" : "sync(other stream)");
    return fail_on == "sync" ? hipErrorLaunchFailure : hipSuccess;
}
extern "C" hipError_t hipFree(void* p)
{
    calls.push_back("free");
    if (fail_on == "free") return hipErrorInvalidValue;
    if (!live.erase(p)) {
        frees_of_dead++;
        return hipErrorInvalidValue;
    }
    std::free(p);
    return hipSuccess;
}
extern "C" hipError_t hipMalloc(void** p, size_t bytes)
{
    calls.push_back("malloc:" + std::to_string(bytes));
    if (injected("malloc")) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    live.insert(*p);
    return hipSuccess;
}
namespace gnsship {
int fail(gnsship_ctx*, int code, const char* what)
{
    last_fail = what;
    return code;
}
int hip_fail(gnsship_ctx*, hipError_t e, const char* where)
{
    last_where = where;
    return e == hipErrorOutOfMemory ? GNSSHIP_E_NOMEM : GNSSHIP_E_DEVICE;
}
}  // namespace gnsship

using gnsship::alloc_all;
using gnsship::copy_out;
using gnsship::dev_alloc;
using gnsship::DevBuf;
using gnsship::free_all;
using gnsship::release;
using gnsship::reserve;

int main()
{
    gnsship_ctx ctx;
    ctx.stream = kStream;
    DevBuf b;
    bool grew = true;

    // nothing asked of an empty buffer, then the first allocation: no free
    EXPECT(reserve(&ctx, b, 0, "f", "x", &grew) == GNSSHIP_OK && !grew && log().empty() && !b.dev && b.cap == 0);
    EXPECT(reserve(&ctx, b, 100, "f", "x", &grew) == GNSSHIP_OK && grew && log() == "sync malloc:100 ");
    EXPECT(b.dev && b.cap == 100 && live.count(b.dev) == 1 && live.size() == 1);
    std::memset(b.as<char>(), 1, 100);  // typed access, and the block is 100 bytes (address sanitizer)
    // enough: smaller, equal, zero; the optional flag may be left out
    void* const first = b.dev;
    EXPECT(reserve(&ctx, b, 40, "f", "x", &grew) == GNSSHIP_OK && !grew && log().empty());
    EXPECT(reserve(&ctx, b, 100, "f", "x", &grew) == GNSSHIP_OK && !grew && log().empty());
    EXPECT(reserve(&ctx, b, 0, "f", "x") == GNSSHIP_OK && log().empty() && b.dev == first && b.cap == 100);
    // a grow: synchronise, free, allocate
    EXPECT(reserve(&ctx, b, 101, "f", "x", &grew) == GNSSHIP_OK && grew && log() == "sync free malloc:101 ");
    EXPECT(b.dev && b.cap == 101 && live.count(b.dev) == 1 && live.size() == 1);

    // an injected failure at each step, from a held buffer; then a fresh allocation
    struct Case {
        const char* step;
        const char* log;
        int rc;
        size_t left_live;  // blocks the failed step could not release
    } const cases[] = {{"sync", "sync ", GNSSHIP_E_DEVICE, 1}, {"free", "sync free ", GNSSHIP_E_DEVICE, 1},
        {"malloc", "sync free malloc:500 ", GNSSHIP_E_NOMEM, 0}};
    for (const Case& c : cases) {
        release(b);
        log();
        EXPECT(live.empty());
        EXPECT(reserve(&ctx, b, 200, "f", "x") == GNSSHIP_OK && log() == "sync malloc:200 ");
        void* const held = b.dev;
        fail_at(c.step);
        grew = true;
        last_where.clear();
        EXPECT(reserve(&ctx, b, 500, "gnsship_entry", "buffer", &grew) == c.rc);
        EXPECT(log() == c.log);
        EXPECT(!grew && b.dev == nullptr && b.cap == 0);
        EXPECT(last_where == "gnsship_entry(buffer)");
        EXPECT(live.size() == c.left_live && (c.left_live == 0 || live.count(held) == 1));
        fail_at("");
        // smaller than what it held before the failure: the stale capacity is gone, so this allocates, and frees nothing
        EXPECT(reserve(&ctx, b, 150, "f", "x", &grew) == GNSSHIP_OK && grew && log() == "sync malloc:150 ");
        EXPECT(b.dev && b.cap == 150 && live.count(b.dev) == 1 && live.size() == c.left_live + 1);
        EXPECT(reserve(&ctx, b, 300, "f", "x", &grew) == GNSSHIP_OK && grew && log() == "sync free malloc:300 ");
        EXPECT(b.dev && b.cap == 300 && live.count(b.dev) == 1 && live.size() == c.left_live + 1);
        if (c.left_live) {  // the block the failed step left behind is the fake's to return
            live.erase(held);
            std::free(held);
        }
    }
    // a first allocation that fails
    release(b);
    log();
    fail_at("malloc");
    EXPECT(reserve(&ctx, b, 64, "f", "x", &grew) == GNSSHIP_E_NOMEM && !grew && !b.dev && b.cap == 0 && log() == "sync malloc:64 ");
    fail_at("");

    // release: once, then nothing
    EXPECT(reserve(&ctx, b, 64, "f", "x") == GNSSHIP_OK);
    log();
    release(b);
    EXPECT(log() == "free " && !b.dev && b.cap == 0 && live.empty());
    release(b);
    EXPECT(log().empty());

    // stage: reserve under `what`, then the copy; a large enough buffer sees the copy alone
    char host[64];
    std::memset(host, 7, sizeof(host));
    EXPECT(gnsship::stage(&ctx, b, host, 48, "gnsship_entry", "stage") == GNSSHIP_OK && log() == "sync malloc:48 h2d:48 ");
    EXPECT(b.cap == 48 && b.as<char>()[47] == 7);
    EXPECT(gnsship::stage(&ctx, b, host, 16, "gnsship_entry", "stage") == GNSSHIP_OK && log() == "h2d:16 ");
    fail_at("h2d");
    last_where.clear();
    EXPECT(gnsship::stage(&ctx, b, host, 16, "gnsship_entry", "stage") == GNSSHIP_E_DEVICE && log() == "h2d:16 " && last_where == "gnsship_entry(upload)");
    EXPECT(b.dev && b.cap == 48);  // a failed copy leaves the buffer as it was
    fail_at("malloc");
    EXPECT(gnsship::stage(&ctx, b, host, 64, "gnsship_entry", "stage") == GNSSHIP_E_NOMEM && log() == "sync free malloc:64 ");
    EXPECT(last_where == "gnsship_entry(stage)" && !b.dev && b.cap == 0 && live.empty());
    fail_at("sync");
    EXPECT(gnsship::stage(&ctx, b, host, 64, "gnsship_f", "upload") == GNSSHIP_E_DEVICE && log() == "sync " && last_where == "gnsship_f(upload)");
    fail_at("");
    EXPECT(gnsship::stage(&ctx, b, host, 64, "gnsship_entry", "stage") == GNSSHIP_OK && log() == "sync malloc:64 h2d:64 ");

    // `room`: what a buffer that has to grow is given; one that is large enough is left alone, whatever the room
    {
        DevBuf r;
        EXPECT(gnsship::stage(&ctx, r, host, 16, "gnsship_entry", "stage", 40) == GNSSHIP_OK && log() == "sync malloc:40 h2d:16 " && r.cap == 40);
        EXPECT(gnsship::stage(&ctx, r, host, 32, "gnsship_entry", "stage", 64) == GNSSHIP_OK && log() == "h2d:32 " && r.cap == 40);
        EXPECT(gnsship::stage(&ctx, r, host, 48, "gnsship_entry", "stage", 40) == GNSSHIP_OK && log() == "sync free malloc:48 h2d:48 " && r.cap == 48);
        release(r);
        log();
    }

    // copy_out: in order, one synchronise; nothing at all for null or empty entries; stops at the first failure
    char out1[8] = {}, out2[4] = {}, out3[2] = {};
    const char* dev = b.as<char>();
    EXPECT(copy_out(&ctx, {{out1, dev, 8}, {nullptr, dev, 8}, {out2, dev, 0}, {out3, dev, 2}, {out2, dev, 4}}, "gnsship_entry(download)") == GNSSHIP_OK);
    EXPECT(log() == "d2h:8 d2h:2 d2h:4 sync " && out1[7] == 7 && out2[3] == 7 && out3[1] == 7);
    EXPECT(copy_out(&ctx, {{nullptr, dev, 8}, {out2, dev, 0}, {nullptr, nullptr, 0}}, "gnsship_entry(download)") == GNSSHIP_OK && log().empty());
    EXPECT(copy_out(&ctx, {}, "gnsship_entry(download)") == GNSSHIP_OK && log().empty());
    const gnsship::DevCopy three[3] = {{out3, dev, 2}, {nullptr, dev, 4}, {out2, dev, 4}};  // an array and a count: the first two only
    EXPECT(copy_out(&ctx, three, 2, "gnsship_entry(download)") == GNSSHIP_OK && log() == "d2h:2 sync ");
    EXPECT(copy_out(&ctx, three + 1, 1, "gnsship_entry(download)") == GNSSHIP_OK && log().empty());
    fail_at("d2h#2");
    last_where.clear();
    EXPECT(copy_out(&ctx, {{out1, dev, 8}, {out3, dev, 2}, {out2, dev, 4}}, "gnsship_entry(download)") == GNSSHIP_E_DEVICE);
    EXPECT(log() == "d2h:8 d2h:2 " && last_where == "gnsship_entry(download)");
    fail_at("sync");
    last_where.clear();
    EXPECT(copy_out(&ctx, {{out1, dev, 8}, {out3, dev, 2}}, "gnsship_entry") == GNSSHIP_E_DEVICE && log() == "d2h:8 d2h:2 sync " && last_where == "gnsship_entry");
    fail_at("");
    release(b);
    log();

    // alloc_all: every allocation, then the memsets that were asked for, each over its whole block
    float* f = nullptr;
    int64_t* q = nullptr;
    uint8_t* u = nullptr;
    EXPECT(alloc_all(&ctx, {dev_alloc(&f, 3, true), dev_alloc(&q, 2), dev_alloc(&u, 5, true)}) == hipSuccess);
    EXPECT(log() == "malloc:12 malloc:16 malloc:5 memset:12 memset:5 " && live.size() == 3 && f[2] == 0.0f && u[4] == 0);
    free_all({f, nullptr, q, u, nullptr});
    EXPECT(log() == "free free free " && live.empty() && frees_of_dead == 0);
    free_all({});
    free_all({nullptr});
    EXPECT(log().empty());
    f = nullptr, q = nullptr, u = nullptr;
    fail_at("malloc#2");
    EXPECT(alloc_all(&ctx, {dev_alloc(&f, 3, true), dev_alloc(&q, 2, true), dev_alloc(&u, 5, true)}) == hipErrorOutOfMemory);
    EXPECT(log() == "malloc:12 malloc:16 " && f && !q && !u && live.size() == 1);  // what a handle's destroy then frees
    free_all({f, q, u});
    EXPECT(log() == "free " && live.empty());
    f = nullptr;
    fail_at("memset#1");
    EXPECT(alloc_all(&ctx, {dev_alloc(&f, 3, true), dev_alloc(&u, 5, true)}) == hipErrorInvalidValue && log() == "malloc:12 malloc:5 memset:12 ");
    fail_at("");
    free_all({f, u});
    EXPECT(log() == "free free " && live.empty());

    // the destroy prologue, and the two texts
    ctx.device = 3;
    gnsship::quiesce(&ctx);
    EXPECT(log() == "device:3 sync ");
    EXPECT(gnsship::reject(&ctx, GNSSHIP_E_STATE, "gnsship_entry", "not now") == GNSSHIP_E_STATE && last_fail == "gnsship_entry: not now");
    EXPECT(gnsship::launched(&ctx, "gnsship_entry(launch)") == GNSSHIP_OK);
    last_error = hipErrorLaunchFailure;
    last_where.clear();
    EXPECT(gnsship::launched(&ctx, "gnsship_entry(launch)") == GNSSHIP_E_DEVICE && last_where == "gnsship_entry(launch)" && log().empty());

    EXPECT(frees_of_dead == 0);
    std::printf("dev_buf_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
