// tlm_mirror_calls_check.cpp — the five telemetry decoder families of include/gnsship_cpp.hpp (Galileo_, Gps_L1_Ca_,
// Gps_Cnav_, Beidou_Dnav_, Glonass_Gnav_Telemetry_Decoder_Hip and the signal-named blocks on them) against a stub of the
// C ABI: no library, no GPU.
//
// The stub defines the C functions that Device, the tracking mirror's constructor and the telemetry classes call.  Every
// call is logged as "name(scalar arguments)[pointer arguments that were null]" with whether the device mutex was held;
// `fail_next` makes the next call fail.  The run functions write everything the C contract lets the library write:
// max_channels · per_run records (and that many · data_length bits), max_channels counts and faults, and
// max_rounds · max_channels tow_ms and sflags — each call with other values, so a stale or undersized vector shows.
//
// Checked (tests/test_tlm_mirror_calls.py runs this under -fsanitize=address,undefined), for every public method of every
// family, with max_channels 3, max_rounds 5 and per_run 2:
//  (a) the C function it calls, its scalar arguments, which pointer arguments are null, under the device mutex, and that
//      the method returns false when the call fails;
//  (b) the output vectors hold the stub's full extent (an undersized one is a sanitizer error), Galileo's bits for each of
//      the data lengths 114, 238 and 486; rounds() is n_rounds after work_symbols / work_records and, for work_trk, the
//      library's n_rounds_out, 0 when that call fails;
//  (c) a failing create throws "<create>: <the stub's error text>"; a signal-named block given the other signal's
//      configuration throws "the configuration's signal is not this block's" before any C call;
//  (d) every signal-named block is created and deleted through a unique_ptr to its family class: destroyed exactly once.
#include <cstdint>
#include <cstdio>
#include <future>
#include <initializer_list>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "gnsship_cpp.hpp"

namespace {
constexpr int32_t C = 3, R = 5, PER_RUN = 2;
struct Handle {
    int32_t channels = 0, max_rounds = 0, data_length = 0;
};
std::set<const void*> live;  // the handles created and not yet destroyed
int destroys = 0;
std::string last;            // the last logged call
bool locked = false;         // ... was made under the device mutex
bool fail_next = false;
int salt = 0;                // changes with every run, so that no run's outputs pass for another's
std::mutex* device_mutex = nullptr;
const char kError[] = "stub says no";
int failures = 0;

void expect(bool ok, const char* what, int line)
{
    if (ok) return;
    std::printf("FAIL line %d: %s (last call: %s%s)\n", line, what, last.c_str(), locked ? "" : ", unlocked");
    failures++;
}
#define EXPECT(c) expect((c), #c, __LINE__)

using Ptrs = std::initializer_list<std::pair<const char*, const void*>>;
int called(const char* name, std::initializer_list<long long> scalars, Ptrs ptrs)
{
    last = std::string(name) + "(";
    for (long long s : scalars) last += (last.back() == '(' ? "" : ",") + std::to_string(s);
    last += ")[";
    for (const auto& p : ptrs)
        if (!p.second) last += (last.back() == '[' ? "" : " ") + std::string(p.first);
    last += "]";
    // std::mutex::try_lock by its owner is undefined: ask from another thread
    locked = device_mutex && std::async(std::launch::async, [] {
        if (!device_mutex->try_lock()) return true;
        device_mutex->unlock();
        return false;
    }).get();
    const bool fail = fail_next;
    fail_next = false;
    return fail ? GNSSHIP_E_INVAL : GNSSHIP_OK;
}

template <class H> int create(const char* name, std::initializer_list<long long> scalars, const void* ctx, const void* conf, int32_t channels,
    int32_t max_rounds, int32_t data_length, H** out)
{
    if (called(name, scalars, {{"ctx", ctx}, {"conf", conf}, {"out", out}}) != GNSSHIP_OK) return GNSSHIP_E_INVAL;
    *out = new H;
    (*out)->channels = channels;
    (*out)->max_rounds = max_rounds;
    (*out)->data_length = data_length;
    live.insert(*out);
    return GNSSHIP_OK;
}
template <class H> int destroy(H* h)
{
    destroys++;
    if (!live.erase(h)) {
        std::printf("FAIL: destroy of a handle that is not live\n");
        failures++;
        return GNSSHIP_E_INVAL;
    }
    delete h;
    return GNSSHIP_OK;
}
template <class T> void fill(T* p, size_t n, long long base)
{
    for (size_t i = 0; p && i < n; i++) p[i] = static_cast<T>(base + salt + static_cast<long long>(i));
}
// a run's outputs, to the full extent of the C contract, wherever a host pointer was given
template <class Rec> void run_outputs(const Handle* h, Rec* recs, uint8_t* bits, int32_t* counts, uint8_t* faults, uint32_t* tow_ms, uint8_t* sflags)
{
    salt++;
    const size_t nc = static_cast<size_t>(h->channels), slots = nc * PER_RUN, entries = nc * static_cast<size_t>(h->max_rounds);
    for (size_t i = 0; recs && i < slots; i++) {
        recs[i] = Rec{};
        recs[i].symbol_counter = 7000 + static_cast<uint64_t>(salt) + i;
    }
    fill(bits, slots * static_cast<size_t>(h->data_length), 0);
    fill(counts, nc, 10);
    fill(faults, nc, 20);
    fill(tow_ms, entries, 3000);
    fill(sflags, entries, 40);
}
}  // namespace

struct gnsship_ctx {};
struct gnsship_trk : Handle {};
struct gnsship_tlm : Handle {};
struct gnsship_lnav : Handle {};
struct gnsship_cnav : Handle {};
struct gnsship_dnav : Handle {};
struct gnsship_gnav : Handle {};

extern "C" {
int gnsship_abi_version(void) { return GNSSHIP_ABI_VERSION; }
int gnsship_ctx_create(int, gnsship_ctx** out)
{
    *out = new gnsship_ctx;
    return GNSSHIP_OK;
}
int gnsship_ctx_destroy(gnsship_ctx* ctx)
{
    delete ctx;
    return GNSSHIP_OK;
}
const char* gnsship_last_error(const gnsship_ctx*) { return kError; }
int gnsship_trk_create(gnsship_ctx* ctx, const gnsship_trk_conf* conf, int max_channels, gnsship_trk** out)
{
    return create("gnsship_trk_create", {max_channels}, ctx, conf, max_channels, 0, 0, out);
}
int gnsship_trk_destroy(gnsship_trk* t) { return destroy(t); }

// ---- Galileo ----
int gnsship_tlm_create(gnsship_ctx* ctx, const gnsship_tlm_conf* c, int32_t max_channels, gnsship_tlm** out)
{
    const int32_t LL = c->frame_type == GNSSHIP_TLM_INAV ? 114 : c->frame_type == GNSSHIP_TLM_FNAV ? 238 : 486;  // gnsship.h's table
    return create("gnsship_tlm_create", {c->frame_type, c->vit_mode, c->max_rounds, c->reserved, max_channels}, ctx, c, max_channels, c->max_rounds, LL, out);
}
int gnsship_tlm_run_symbols(gnsship_tlm* t, const float* symbols, const uint8_t* valid, int on_device, int32_t n_rounds, gnsship_tlm_page* pages,
    uint8_t* bits, int32_t* counts, uint8_t* faults)
{
    const int rc = called("gnsship_tlm_run_symbols", {on_device, n_rounds},
        {{"t", t}, {"symbols", symbols}, {"valid", valid}, {"pages", pages}, {"bits", bits}, {"counts", counts}, {"faults", faults}});
    if (rc == GNSSHIP_OK) run_outputs(t, pages, bits, counts, faults, nullptr, nullptr);
    return rc;
}
int gnsship_tlm_run_records(gnsship_tlm* t, const gnsship_trk_epoch* records, int on_device, int32_t n_rounds, gnsship_tlm_page* pages, uint8_t* bits,
    int32_t* counts, uint8_t* faults)
{
    const int rc = called("gnsship_tlm_run_records", {on_device, n_rounds},
        {{"t", t}, {"records", records}, {"pages", pages}, {"bits", bits}, {"counts", counts}, {"faults", faults}});
    if (rc == GNSSHIP_OK) run_outputs(t, pages, bits, counts, faults, nullptr, nullptr);
    return rc;
}
int gnsship_tlm_run_trk(gnsship_tlm* t, gnsship_trk* trk, gnsship_tlm_page* pages, uint8_t* bits, int32_t* counts, uint8_t* faults)
{
    const int rc = called("gnsship_tlm_run_trk", {static_cast<long long>(live.count(trk))},
        {{"t", t}, {"trk", trk}, {"pages", pages}, {"bits", bits}, {"counts", counts}, {"faults", faults}});
    if (rc == GNSSHIP_OK) run_outputs(t, pages, bits, counts, faults, nullptr, nullptr);
    return rc;
}
int gnsship_tlm_outputs_device(gnsship_tlm*, gnsship_tlm_page**, uint8_t**, int32_t**, uint8_t**, int32_t* per_run)
{
    if (per_run) *per_run = PER_RUN;
    return GNSSHIP_OK;
}
int gnsship_tlm_reset_channel(gnsship_tlm* t, int32_t channel) { return called("gnsship_tlm_reset_channel", {channel}, {{"t", t}}); }
int gnsship_tlm_set_satellite(gnsship_tlm* t, int32_t channel) { return called("gnsship_tlm_set_satellite", {channel}, {{"t", t}}); }
int gnsship_tlm_new_channel(gnsship_tlm* t, int32_t channel) { return called("gnsship_tlm_new_channel", {channel}, {{"t", t}}); }
int gnsship_tlm_state_get(gnsship_tlm* t, int32_t channel, gnsship_tlm_state* st)
{
    st->symbol_counter = 900 + static_cast<uint64_t>(channel);
    return called("gnsship_tlm_state_get", {channel}, {{"t", t}, {"st", st}});
}
int gnsship_tlm_destroy(gnsship_tlm* t) { return destroy(t); }

// ---- the four families with a TOW stream.  second: the configuration's second field; third: the name of run_symbols'
// third input; the FAULTS_* arguments: the faults parameter, its value and its log entry, or nothing for a family without ----
#define STREAM_FAMILY(fam, rec_t, second, third, FAULTS_PARAM, FAULTS_ARG, FAULTS_LOG)                                                                         \
    int gnsship_##fam##_create(gnsship_ctx* ctx, const gnsship_##fam##_conf* c, int32_t max_channels, gnsship_##fam** out)                           \
    {                                                                                                                                                 \
        return create("gnsship_" #fam "_create", {c->max_rounds, c->second, max_channels}, ctx, c, max_channels, c->max_rounds, 0, out);        \
    }                                                                                                                                                 \
    int gnsship_##fam##_run_symbols(gnsship_##fam* t, const float* symbols, const uint8_t* valid, const uint8_t* third, int on_device,               \
        int32_t n_rounds, rec_t* recs, int32_t* counts, FAULTS_PARAM uint32_t* tow_ms, uint8_t* sflags)                                               \
    {                                                                                                                                                 \
        const int rc = called("gnsship_" #fam "_run_symbols", {on_device, n_rounds},                                                                  \
            {{"t", t}, {"symbols", symbols}, {"valid", valid}, {#third, third}, {"recs", recs}, {"counts", counts}, FAULTS_LOG{"tow_ms", tow_ms},     \
                {"sflags", sflags}});                                                                                                                 \
        if (rc == GNSSHIP_OK) run_outputs(t, recs, nullptr, counts, FAULTS_ARG, tow_ms, sflags);                                                      \
        return rc;                                                                                                                                    \
    }                                                                                                                                                 \
    int gnsship_##fam##_run_records(gnsship_##fam* t, const gnsship_trk_epoch* records, int on_device, int32_t n_rounds, rec_t* recs,                \
        int32_t* counts, FAULTS_PARAM uint32_t* tow_ms, uint8_t* sflags)                                                                              \
    {                                                                                                                                                 \
        const int rc = called("gnsship_" #fam "_run_records", {on_device, n_rounds},                                                                  \
            {{"t", t}, {"records", records}, {"recs", recs}, {"counts", counts}, FAULTS_LOG{"tow_ms", tow_ms}, {"sflags", sflags}});                  \
        if (rc == GNSSHIP_OK) run_outputs(t, recs, nullptr, counts, FAULTS_ARG, tow_ms, sflags);                                                      \
        return rc;                                                                                                                                    \
    }                                                                                                                                                 \
    int gnsship_##fam##_run_trk(gnsship_##fam* t, gnsship_trk* trk, rec_t* recs, int32_t* counts, FAULTS_PARAM uint32_t* tow_ms, uint8_t* sflags,    \
        int32_t* n_rounds_out)                                                                                                                        \
    {                                                                                                                                                 \
        const int rc = called("gnsship_" #fam "_run_trk", {static_cast<long long>(live.count(trk))},                                                  \
            {{"t", t}, {"trk", trk}, {"recs", recs}, {"counts", counts}, FAULTS_LOG{"tow_ms", tow_ms}, {"sflags", sflags},                            \
                {"n_rounds_out", n_rounds_out}});                                                                                                     \
        if (rc != GNSSHIP_OK) return rc; /* and n_rounds_out is not written */                                                                        \
        run_outputs(t, recs, nullptr, counts, FAULTS_ARG, tow_ms, sflags);                                                                            \
        if (n_rounds_out) *n_rounds_out = t->max_rounds;                                                                                              \
        return rc;                                                                                                                                    \
    }                                                                                                                                                 \
    int gnsship_##fam##_state_get(gnsship_##fam* t, int32_t channel, gnsship_##fam##_state* st)                                                      \
    {                                                                                                                                                 \
        st->symbol_counter = 900 + static_cast<uint64_t>(channel);                                                                                    \
        return called("gnsship_" #fam "_state_get", {channel}, {{"t", t}, {"st", st}});                                                               \
    }                                                                                                                                                 \
    int gnsship_##fam##_destroy(gnsship_##fam* t) { return destroy(t); }
#define NOTHING
#define COMMA ,
STREAM_FAMILY(lnav, gnsship_lnav_subframe, reserved, flags180, uint8_t* faults COMMA, faults, {"faults" COMMA faults} COMMA)
STREAM_FAMILY(cnav, gnsship_cnav_message, signal, out_valid, uint8_t* faults COMMA, faults, {"faults" COMMA faults} COMMA)
STREAM_FAMILY(dnav, gnsship_dnav_subframe, signal, out_valid, NOTHING, nullptr, NOTHING)
STREAM_FAMILY(gnav, gnsship_gnav_string, signal, out_valid, NOTHING, nullptr, NOTHING)

int gnsship_lnav_outputs_device(gnsship_lnav*, gnsship_lnav_subframe**, int32_t**, uint8_t**, uint32_t**, uint8_t**, int32_t* per_run)
{
    if (per_run) *per_run = PER_RUN;
    return GNSSHIP_OK;
}
int gnsship_cnav_outputs_device(gnsship_cnav*, gnsship_cnav_message**, int32_t**, uint8_t**, uint32_t**, uint8_t**, int32_t* per_run)
{
    if (per_run) *per_run = PER_RUN;
    return GNSSHIP_OK;
}
int gnsship_dnav_outputs_device(gnsship_dnav*, gnsship_dnav_subframe**, int32_t**, uint32_t**, uint8_t**, int32_t* per_run)
{
    if (per_run) *per_run = PER_RUN;
    return GNSSHIP_OK;
}
int gnsship_gnav_outputs_device(gnsship_gnav*, gnsship_gnav_string**, int32_t**, uint32_t**, uint8_t**, int32_t* per_run)
{
    if (per_run) *per_run = PER_RUN;
    return GNSSHIP_OK;
}
int gnsship_lnav_reset_channel(gnsship_lnav* t, int32_t channel) { return called("gnsship_lnav_reset_channel", {channel}, {{"t", t}}); }
int gnsship_lnav_set_satellite(gnsship_lnav* t, int32_t channel) { return called("gnsship_lnav_set_satellite", {channel}, {{"t", t}}); }
int gnsship_lnav_new_channel(gnsship_lnav* t, int32_t channel) { return called("gnsship_lnav_new_channel", {channel}, {{"t", t}}); }
int gnsship_cnav_reset_channel(gnsship_cnav* t, int32_t channel) { return called("gnsship_cnav_reset_channel", {channel}, {{"t", t}}); }
int gnsship_cnav_new_channel(gnsship_cnav* t, int32_t channel) { return called("gnsship_cnav_new_channel", {channel}, {{"t", t}}); }
int gnsship_cnav_state_set(gnsship_cnav* t, int32_t channel, const gnsship_cnav_state* st)
{
    return called("gnsship_cnav_state_set", {channel, static_cast<long long>(st ? st->symbol_counter : 0)}, {{"t", t}, {"st", st}});
}
int gnsship_dnav_reset_channel(gnsship_dnav* t, int32_t channel) { return called("gnsship_dnav_reset_channel", {channel}, {{"t", t}}); }
int gnsship_dnav_set_satellite(gnsship_dnav* t, int32_t channel, int32_t prn) { return called("gnsship_dnav_set_satellite", {channel, prn}, {{"t", t}}); }
int gnsship_dnav_new_channel(gnsship_dnav* t, int32_t channel, int32_t prn) { return called("gnsship_dnav_new_channel", {channel, prn}, {{"t", t}}); }
int gnsship_gnav_set_satellite(gnsship_gnav* t, int32_t channel, int32_t prn) { return called("gnsship_gnav_set_satellite", {channel, prn}, {{"t", t}}); }
int gnsship_gnav_new_channel(gnsship_gnav* t, int32_t channel, int32_t prn) { return called("gnsship_gnav_new_channel", {channel, prn}, {{"t", t}}); }
int gnsship_gnav_state_set(gnsship_gnav* t, int32_t channel, const gnsship_gnav_state* st)
{
    return called("gnsship_gnav_state_set", {channel, static_cast<long long>(st ? st->symbol_counter : 0)}, {{"t", t}, {"st", st}});
}
}  // extern "C"

namespace {
using namespace gnsship;

// (a) one bool method: the call it logs, under the device mutex; false when that call fails
template <class F> void check_call(F&& f, const std::string& want, int line)
{
    last.clear();
    locked = false;
    const bool ok = f();
    expect(ok, "the method returns true", line);
    expect(last == want, ("the call is " + want).c_str(), line);
    expect(locked, "under the device mutex", line);
    fail_next = true;
    expect(!f(), "false when the C call fails", line);
    expect(!fail_next, "the failing call was made", line);
    fail_next = false;
}
#define CALL(expr, want) check_call([&] { return (expr); }, want, __LINE__)

// (b) a vector holds the n values the last run wrote from `base` on
template <class T> void check_filled(const std::vector<T>& v, size_t n, long long base, int line)
{
    bool ok = v.size() == n;
    for (size_t i = 0; ok && i < n; i++) ok = v[i] == static_cast<T>(base + salt + static_cast<long long>(i));
    expect(ok, "the vector holds the run's full extent", line);
}
template <class Rec> void check_records(const std::vector<Rec>& v, int line)
{
    bool ok = v.size() == static_cast<size_t>(C) * PER_RUN;
    for (size_t i = 0; ok && i < v.size(); i++) ok = v[i].symbol_counter == 7000 + static_cast<uint64_t>(salt) + i;
    expect(ok, "the records hold the run's full extent", line);
}
// the TOW stream of a run and rounds()
template <class D> void check_stream(const D& d, int32_t rounds, int line)
{
    check_filled(d.counts(), C, 10, line);
    check_filled(d.tow_ms(), static_cast<size_t>(R) * C, 3000, line);
    check_filled(d.sflags(), static_cast<size_t>(R) * C, 40, line);
    expect(d.rounds() == rounds, "rounds()", line);
}
// (c) the constructor refuses with this text, and makes `calls` C calls ("" = none) on the way
template <class F> void check_throws(F&& make, const std::string& text, const std::string& call, bool fail_create, int line)
{
    const size_t live_before = live.size();
    std::string what = "(no exception)";
    last.clear();
    fail_next = fail_create;
    try {
        make();
    } catch (const std::invalid_argument& e) {
        what = e.what();
    }
    fail_next = false;
    expect(what == text, ("throws std::invalid_argument: " + text + ", got: " + what).c_str(), line);
    expect(last.compare(0, call.size(), call) == 0 && (!call.empty() || last.empty()), "the C calls of a refused constructor", line);
    expect(live.size() == live_before, "a refused constructor leaves no handle", line);
}
// (d) destroyed exactly once when the owner lets go
template <class P> void check_destroyed_once(P& p, int line)
{
    const int before = destroys;
    const size_t live_before = live.size();
    p.reset();
    expect(destroys == before + 1 && live.size() + 1 == live_before, "destroyed exactly once", line);
}

const float kSymbols[R * C] = {};
const uint8_t kFlags[R * C] = {};
const gnsship_trk_epoch kRecords[R * C] = {};

void check_galileo(const gnsship_tlm_conf& conf, int32_t LL, const Dll_Pll_Veml_Tracking_Hip& trk)
{
    const std::string create = "gnsship_tlm_create(" + std::to_string(conf.frame_type) + "," + std::to_string(conf.vit_mode) + ",5,0,3)[]";
    check_throws([&] { Galileo_Telemetry_Decoder_Hip d(conf, C); }, std::string("gnsship_tlm_create: ") + kError, create, true, __LINE__);
    last.clear();
    auto d = std::make_unique<Galileo_Telemetry_Decoder_Hip>(conf, C);
    EXPECT(last == create && locked);
    EXPECT(d->data_length() == LL && d->pages_per_run() == PER_RUN);
    EXPECT(d->last_error() == kError);
    CALL(d->set_satellite(1), "gnsship_tlm_set_satellite(1)[]");
    CALL(d->reset(2), "gnsship_tlm_reset_channel(2)[]");
    CALL(d->new_channel(0), "gnsship_tlm_new_channel(0)[]");
    auto outputs = [&](int line) {
        check_records(d->pages(), line);
        check_filled(d->bits(), static_cast<size_t>(C) * PER_RUN * static_cast<size_t>(LL), 0, line);
        check_filled(d->counts(), C, 10, line);
        check_filled(d->faults(), C, 20, line);
    };
    CALL(d->work_symbols(kSymbols, nullptr, R), "gnsship_tlm_run_symbols(0,5)[valid]");
    CALL(d->work_symbols(kSymbols, kFlags, 3, true), "gnsship_tlm_run_symbols(1,3)[]");
    outputs(__LINE__);
    CALL(d->work_records(kRecords, R), "gnsship_tlm_run_records(0,5)[]");
    CALL(d->work_records(kRecords, 3, true), "gnsship_tlm_run_records(1,3)[]");
    outputs(__LINE__);
    CALL(d->work_trk(trk), "gnsship_tlm_run_trk(1)[]");
    outputs(__LINE__);
    last.clear();
    EXPECT(d->state(2).symbol_counter == 902 && last == "gnsship_tlm_state_get(2)[]" && locked);
    check_destroyed_once(d, __LINE__);
}

void check_lnav(const Dll_Pll_Veml_Tracking_Hip& trk)
{
    const gnsship_lnav_conf conf = gps_l1_ca_tlm_conf(R);
    check_throws([&] { Gps_L1_Ca_Telemetry_Decoder_Hip d(conf, C); }, std::string("gnsship_lnav_create: ") + kError, "gnsship_lnav_create(5,0,3)[]", true,
        __LINE__);
    last.clear();
    auto d = std::make_unique<Gps_L1_Ca_Telemetry_Decoder_Hip>(conf, C);
    EXPECT(last == "gnsship_lnav_create(5,0,3)[]" && locked);
    EXPECT(d->subframes_per_run() == PER_RUN && d->rounds() == 0);
    EXPECT(d->last_error() == kError);
    CALL(d->set_satellite(1), "gnsship_lnav_set_satellite(1)[]");
    CALL(d->reset(2), "gnsship_lnav_reset_channel(2)[]");
    CALL(d->new_channel(0), "gnsship_lnav_new_channel(0)[]");
    auto outputs = [&](int32_t rounds, int line) {
        check_records(d->subframes(), line);
        check_filled(d->faults(), C, 20, line);
        check_stream(*d, rounds, line);
    };
    CALL(d->work_symbols(kSymbols, nullptr, nullptr, 3), "gnsship_lnav_run_symbols(0,3)[valid flags180]");
    CALL(d->work_symbols(kSymbols, kFlags, nullptr, 3), "gnsship_lnav_run_symbols(0,3)[flags180]");
    CALL(d->work_symbols(kSymbols, nullptr, kFlags, 3), "gnsship_lnav_run_symbols(0,3)[valid]");
    outputs(3, __LINE__);
    CALL(d->work_symbols(kSymbols, kFlags, kFlags, R, true), "gnsship_lnav_run_symbols(1,5)[]");
    outputs(R, __LINE__);
    CALL(d->work_records(kRecords, 3), "gnsship_lnav_run_records(0,3)[]");
    outputs(3, __LINE__);
    CALL(d->work_records(kRecords, R, true), "gnsship_lnav_run_records(1,5)[]");
    outputs(R, __LINE__);
    EXPECT(d->work_records(kRecords, 3));
    CALL(d->work_trk(trk), "gnsship_lnav_run_trk(1)[]");
    EXPECT(d->rounds() == 0);  // CALL ends with the failing call: rounds() is 0 until the library says otherwise
    EXPECT(d->work_trk(trk));
    outputs(R, __LINE__);  // the stub's n_rounds_out is max_rounds
    last.clear();
    EXPECT(d->state(2).symbol_counter == 902 && last == "gnsship_lnav_state_get(2)[]" && locked);
    check_destroyed_once(d, __LINE__);
}

// The three families whose blocks are named by signal: Family the family class, Block / Other its two blocks, conf / other
// their configurations.  Everything goes through a unique_ptr to the family class, as the receiver holds its decoders.
template <class Family, class Block, class Other, class Conf, class Extra>
void check_signal_family(const std::string& fam, const Conf& conf, const Conf& other, const Dll_Pll_Veml_Tracking_Hip& trk, Extra&& extra)
{
    const std::string g = "gnsship_" + fam + "_", create = g + "create(5," + std::to_string(conf.signal) + ",3)[]";
    check_throws([&] { Block d(conf, C); }, g + "create: " + kError, create, true, __LINE__);
    check_throws([&] { Family d(conf, C); }, g + "create: " + kError, create, true, __LINE__);
    check_throws([&] { Block d(other, C); }, "the configuration's signal is not this block's", "", false, __LINE__);
    check_throws([&] { Other d(conf, C); }, "the configuration's signal is not this block's", "", false, __LINE__);
    {
        std::unique_ptr<Family> o = std::make_unique<Other>(other, C);  // (d) for the other block
        EXPECT(o->conf().signal == other.signal);
        check_destroyed_once(o, __LINE__);
        std::unique_ptr<Family> f = std::make_unique<Family>(other, C);  // the family class is a block of either signal
        EXPECT(f->conf().signal == other.signal);
        check_destroyed_once(f, __LINE__);
    }
    last.clear();
    std::unique_ptr<Family> d = std::make_unique<Block>(conf, C);
    EXPECT(last == create && locked);
    EXPECT(d->conf().max_rounds == R && d->conf().signal == conf.signal && d->rounds() == 0);
    EXPECT(d->last_error() == kError);
    auto outputs = [&](int32_t rounds, int line) {
        extra(*d, line);  // the family's records, and its faults if it has them
        check_stream(*d, rounds, line);
    };
    CALL(d->work_symbols(kSymbols, nullptr, nullptr, 3), g + "run_symbols(0,3)[valid out_valid]");
    CALL(d->work_symbols(kSymbols, kFlags, nullptr, 3), g + "run_symbols(0,3)[out_valid]");
    CALL(d->work_symbols(kSymbols, nullptr, kFlags, 3), g + "run_symbols(0,3)[valid]");
    outputs(3, __LINE__);
    CALL(d->work_symbols(kSymbols, kFlags, kFlags, R, true), g + "run_symbols(1,5)[]");
    outputs(R, __LINE__);
    CALL(d->work_records(kRecords, 3), g + "run_records(0,3)[]");
    outputs(3, __LINE__);
    CALL(d->work_records(kRecords, R, true), g + "run_records(1,5)[]");
    outputs(R, __LINE__);
    EXPECT(d->work_records(kRecords, 3));
    CALL(d->work_trk(trk), g + "run_trk(1)[]");
    EXPECT(d->rounds() == 0);
    EXPECT(d->work_trk(trk));
    outputs(R, __LINE__);
    last.clear();
    EXPECT(d->state(2).symbol_counter == 902 && last == g + "state_get(2)[]" && locked);
    check_destroyed_once(d, __LINE__);
}

void check_all()
{
    Dll_Pll_Veml_Tracking_Hip trk(Dll_Pll_Conf{}, C);
    check_galileo(galileo_inav_tlm_conf(R), 114, trk);
    check_galileo(galileo_fnav_tlm_conf(R, GNSSHIP_VIT_MODE_FULL), 238, trk);
    check_galileo(galileo_cnav_tlm_conf(R), 486, trk);
    check_lnav(trk);

    auto cnav = [](Gps_Cnav_Telemetry_Decoder_Hip& d, int line) {
        EXPECT(d.messages_per_run() == PER_RUN);
        check_records(d.messages(), line);
        check_filled(d.faults(), C, 20, line);
        if (d.rounds() != 3) return;  // the per-channel calls once
        CALL(d.reset(2), "gnsship_cnav_reset_channel(2)[]");
        CALL(d.new_channel(0), "gnsship_cnav_new_channel(0)[]");
        gnsship_cnav_state st{};
        st.symbol_counter = 77;
        CALL(d.set_state(1, st), "gnsship_cnav_state_set(1,77)[]");
    };
    check_signal_family<Gps_Cnav_Telemetry_Decoder_Hip, Gps_L2c_Telemetry_Decoder_Hip, Gps_L5_Telemetry_Decoder_Hip>("cnav", gps_l2c_tlm_conf(R),
        gps_l5_tlm_conf(R), trk, cnav);
    check_signal_family<Gps_Cnav_Telemetry_Decoder_Hip, Gps_L5_Telemetry_Decoder_Hip, Gps_L2c_Telemetry_Decoder_Hip>("cnav", gps_l5_tlm_conf(R),
        gps_l2c_tlm_conf(R), trk, cnav);

    auto dnav = [](Beidou_Dnav_Telemetry_Decoder_Hip& d, int line) {
        EXPECT(d.subframes_per_run() == PER_RUN);
        check_records(d.subframes(), line);
        if (d.rounds() != 3) return;
        CALL(d.reset(2), "gnsship_dnav_reset_channel(2)[]");
        CALL(d.set_satellite(1, 17), "gnsship_dnav_set_satellite(1,17)[]");
        CALL(d.new_channel(0, 63), "gnsship_dnav_new_channel(0,63)[]");
    };
    check_signal_family<Beidou_Dnav_Telemetry_Decoder_Hip, Beidou_B1i_Telemetry_Decoder_Hip, Beidou_B3i_Telemetry_Decoder_Hip>("dnav",
        beidou_b1i_tlm_conf(R), beidou_b3i_tlm_conf(R), trk, dnav);
    check_signal_family<Beidou_Dnav_Telemetry_Decoder_Hip, Beidou_B3i_Telemetry_Decoder_Hip, Beidou_B1i_Telemetry_Decoder_Hip>("dnav",
        beidou_b3i_tlm_conf(R), beidou_b1i_tlm_conf(R), trk, dnav);

    auto gnav = [](Glonass_Gnav_Telemetry_Decoder_Hip& d, int line) {
        EXPECT(d.strings_per_run() == PER_RUN);
        check_records(d.strings(), line);
        if (d.rounds() != 3) return;
        CALL(d.set_satellite(1, 17), "gnsship_gnav_set_satellite(1,17)[]");
        CALL(d.new_channel(0, 24), "gnsship_gnav_new_channel(0,24)[]");
        gnsship_gnav_state st{};
        st.symbol_counter = 77;
        CALL(d.set_state(1, st), "gnsship_gnav_state_set(1,77)[]");
    };
    check_signal_family<Glonass_Gnav_Telemetry_Decoder_Hip, Glonass_L1_Ca_Telemetry_Decoder_Hip, Glonass_L2_Ca_Telemetry_Decoder_Hip>("gnav",
        glonass_l1_ca_tlm_conf(R), glonass_l2_ca_tlm_conf(R), trk, gnav);
    check_signal_family<Glonass_Gnav_Telemetry_Decoder_Hip, Glonass_L2_Ca_Telemetry_Decoder_Hip, Glonass_L1_Ca_Telemetry_Decoder_Hip>("gnav",
        glonass_l2_ca_tlm_conf(R), glonass_l1_ca_tlm_conf(R), trk, gnav);
}
}  // namespace

int main()
{
    {
        const std::shared_ptr<gnsship::Device> dev = gnsship::Device::get(0);
        device_mutex = &dev->mutex();
        check_all();
        device_mutex = nullptr;
    }
    EXPECT(live.empty());
    std::printf("tlm_mirror_calls_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
