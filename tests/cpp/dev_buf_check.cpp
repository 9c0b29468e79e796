// dev_buf_check.cpp — the contract of gnsship::reserve / release (csrc/host_api.h) against a fake HIP runtime.
//
// Built without the HIP runtime: hipStreamSynchronize, hipFree, hipMalloc, fail and hip_fail are defined here.  The fakes
// log every call, hand out real host blocks (so the address sanitizer sees a double free or a leak of the fake's own),
// keep the set of live allocations, and fail the call whose name is in `fail_on`.
//
// Checked (tests/test_dev_buf.py runs this under -fsanitize=address,undefined):
//  * enough capacity: no HIP call, not "grew";
//  * a grow: synchronise, free (only when there is an old buffer), allocate, in that order; "grew"; cap = the request;
//  * an injected failure of each of the three steps: the buffer is {nullptr, 0}, nothing after the failed step ran,
//    hip_fail got "<who>(<what>)" and the code it returned is reserve's, not "grew", nothing is freed twice.  A failed
//    allocation leaves no live block.  A failed synchronise or free stops before the old block could be released: that
//    block — and only that — stays live (the stream or the allocator is in error; the handle's destroy would not do better);
//  * a reserve after each failure allocates afresh without a free;
//  * release frees once, empties the buffer, and is a no-op on an empty one.
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
std::string fail_on, last_where;
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
    if (fail_on == "malloc") return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    live.insert(*p);
    return hipSuccess;
}
namespace gnsship {
int fail(gnsship_ctx*, int code, const char*) { return code; }
int hip_fail(gnsship_ctx*, hipError_t e, const char* where)
{
    last_where = where;
    return e == hipErrorOutOfMemory ? GNSSHIP_E_NOMEM : GNSSHIP_E_DEVICE;
}
}  // namespace gnsship

using gnsship::DevBuf;
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
        fail_on = c.step;
        grew = true;
        last_where.clear();
        EXPECT(reserve(&ctx, b, 500, "gnsship_entry", "buffer", &grew) == c.rc);
        EXPECT(log() == c.log);
        EXPECT(!grew && b.dev == nullptr && b.cap == 0);
        EXPECT(last_where == "gnsship_entry(buffer)");
        EXPECT(live.size() == c.left_live && (c.left_live == 0 || live.count(held) == 1));
        fail_on.clear();
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
    fail_on = "malloc";
    EXPECT(reserve(&ctx, b, 64, "f", "x", &grew) == GNSSHIP_E_NOMEM && !grew && !b.dev && b.cap == 0 && log() == "sync malloc:64 ");
    fail_on.clear();

    // release: once, then nothing
    EXPECT(reserve(&ctx, b, 64, "f", "x") == GNSSHIP_OK);
    log();
    release(b);
    EXPECT(log() == "free " && !b.dev && b.cap == 0 && live.empty());
    release(b);
    EXPECT(log().empty());
    EXPECT(frees_of_dead == 0);
    std::printf("dev_buf_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
