// tlm_gps_lnav.hip — gps_l1_ca_telemetry_decoder_gs (gps_l1_ca_telemetry_decoder_gs.cc) on the device up to the time of
// week (include/gnsship.h, gnsship_lnav_*): preamble seeding, the 300-symbol history, check_tlm_separation, the two-state
// frame synchronisation with its 180° flag, decode_subframe with the parity check of :191-214, the subframe ID and TOW of
// the HOW, the parity-error counter, loss of sync and the TOW stamp of every symbol.  Input: floats with a validity mask
// and 180° flags, or tracking's epoch records (host, device, or in place where gnsship_trk left them).  Output: one
// record per decoded subframe, the block's output stream (tow_ms, sflags) per entry, and per-channel fault flags.
//
// Layout: one workgroup of one wavefront per channel, as tlm_galileo.hip and for its reason: a channel's symbols are
// strictly ordered and the machine's next step depends on the last verdict.  No float arithmetic: the block only ever
// asks `x < 0` and `x > 0` of a symbol, so an entry is one of three codes — 0 (zero, −0, NaN: both tests false), 1 (> 0),
// 2 (< 0) — and NaN and ±0 behave exactly as in the block.
//   history  in HBM two 300-bit strings per channel (neg, pos; bit i is the i-th oldest entry), 80 bytes.  For the run
//            they are unpacked into a linear LDS buffer of codes, oldest first, and packed again once at the end
//            (tlm_device.h, shared with tlm_bds_dnav.hip).
//   gather   64 entries at a time; a ballot of the valid entries and a prefix popcount give each symbol its ordinal, and
//            the chunk's n symbols are appended at buf[size .. size + n).  The buffer is linear, not a ring: the history
//            after the chunk's k-th symbol is the 300 entries ending at buf[size + k], whatever was appended behind it, so
//            nothing has to be cut where a subframe falls due.  After the chunk the newest 300 entries move down.
//   seeding  the history is empty only at the start of a run (a new object, or after reset), so the 8 preamble values go
//            in ahead of the first chunk that holds a symbol, under that symbol's 180° flag, and the counter grows by 8.
//   hits     state 0 only, full history only: lane k forms the sign pattern of the 8 oldest entries as they stand after
//            the chunk's k-th symbol; two ballots say all-match / all-mismatch.
//   machine  wave-uniform: state 0 walks the hit ballot with find-first-set, state 1 jumps to the due symbol
//            (counter >= preamble_index + 300).  Between two such symbols nothing but the TOW moves, by 20 ms a symbol.
//            check_tlm_separation is a comparison against a bound that only a good subframe moves, so one test ahead of
//            each decode and one per chunk equal one per symbol.
//   decode   one lane per word: 30 codes to bits under the polarity, D29* / D30* from the raw bits of the lane below
//            (XOR with 0x3FFFFFC0 leaves bits 0 and 1 alone, so only word 1 needs the stored previous word), the
//            rotate-and-mask parity, and a ballot joins the ten verdicts.
//   outputs  every lane keeps the tow_ms / sflags of its own entry: base + 20 · (distance from the last stamping symbol),
//            written once per chunk.
// Every LDS and HBM index comes from lane numbers, sizes and ballot bits, never from a symbol's value.
// The host path around the kernel (staging, the run calls' checks, output copies) is tlm_host.h.
#include <new>

#include "tlm_device.h"
#include "tlm_host.h"

using namespace gnsship;

namespace {

constexpr int kLnavBits = 300;                  // GPS_SUBFRAME_BITS: history capacity, required symbols, period
constexpr int kLnavPre = 8;                     // GPS_CA_PREAMBLE_LENGTH_BITS
constexpr uint32_t kLnavPreZeroMask = 0x2Eu;    // "10001011": bit i set where preamble[i] is '0' (−1)
constexpr uint32_t kLnavPreOneMask = 0xD1u;
constexpr int kLnavCrcErrorLimit = 2;           // :539
constexpr uint64_t kLnavMaxWithoutValid = 6000; // d_required_symbols * 20 (:122)
constexpr int kLnavBuf = 384;                   // 300 + 8 seeded + 64 appended = 372, rounded up
constexpr int kLnavHistWords = 10;              // 300 bits

struct LnavChan {  // one block object's members
    gnsship_lnav_state st;
    uint32_t neg[kLnavHistWords], pos[kLnavHistWords];
};
static_assert(sizeof(LnavChan) == 144, "LnavChan");

struct LnavArgs {
    const float* sym;              // n_rounds × max_channels, or null
    const uint8_t* valid;          // the same shape, or null
    const uint8_t* flags180;       // the same shape, or null
    const gnsship_trk_epoch* rec;  // the same shape, or null (then sym)
    LnavChan* chans;
    gnsship_lnav_subframe* subframes;  // max_channels × subframes_per_run
    int32_t* counts;
    uint8_t* faults;
    uint32_t* tow_ms;              // max_rounds × max_channels
    uint8_t* sflags;               // the same shape
    int32_t max_channels, n_rounds, subframes_per_run;
};

__device__ __forceinline__ uint32_t lnav_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

// gps_word_parityCheck (:191-214)
__device__ __forceinline__ bool lnav_parity(uint32_t w)
{
    const uint32_t t = (w & 0xFBFFBF00u) ^ (lnav_rotl(w, 1) & 0x07FFBF01u) ^ (lnav_rotl(w, 2) & 0xFC0F8100u) ^ (lnav_rotl(w, 3) & 0xF81FFE02u) ^
        (lnav_rotl(w, 4) & 0xFC00000Eu) ^ (lnav_rotl(w, 5) & 0x07F00001u) ^ (lnav_rotl(w, 6) & 0x00003000u);
    const uint32_t parity = (t ^ lnav_rotl(t, 6) ^ lnav_rotl(t, 12) ^ lnav_rotl(t, 18) ^ lnav_rotl(t, 24)) & 0x3Fu;
    return parity == (w & 0x3Fu);
}

__global__ __launch_bounds__(64) void lnav_kernel(const LnavArgs a)
{
    __shared__ uint8_t buf[kLnavBuf];
    const int lane = threadIdx.x;
    const int c = blockIdx.x;  // the grid is max_channels workgroups

    LnavChan* cs = a.chans + c;
    uint64_t counter = tlm_uniform64(cs->st.symbol_counter), preamble_index = tlm_uniform64(cs->st.preamble_index);
    uint64_t last_valid = tlm_uniform64(cs->st.last_valid_preamble), tried = tlm_uniform64(cs->st.subframes_tried);
    uint32_t prev_word = tlm_uniform(cs->st.prev_word), tow_pre = tlm_uniform(cs->st.tow_at_preamble_ms);
    uint32_t tow_cur = tlm_uniform(cs->st.tow_at_current_symbol_ms), nav_tow = tlm_uniform(cs->st.nav_tow_s);
    int stat = tlm_uniform(cs->st.stat) != 0 ? 1 : 0, crc_err = tlm_uniform(cs->st.crc_error_counter);
    int size = min(max(tlm_uniform(cs->st.history_size), 0), kLnavBits);
    bool pll180 = tlm_uniform(static_cast<int>(cs->st.pll_180)) != 0, frame_sync = tlm_uniform(static_cast<int>(cs->st.frame_sync)) != 0;
    bool tow_set = tlm_uniform(static_cast<int>(cs->st.tow_set)) != 0, sent = tlm_uniform(static_cast<int>(cs->st.sent_tlm_failed)) != 0;

    tlm_codes_unpack(buf, kLnavBuf, cs->neg, cs->pos, size, lane);  // the bit strings → codes, oldest first
    __syncthreads();

    int count = 0;
    bool fault = false;
    for (int base = 0; base < a.n_rounds; base += 64) {
        const int r = base + lane;
        const bool in_run = r < a.n_rounds;
        const size_t e = static_cast<size_t>(in_run ? r : 0) * a.max_channels + c;
        bool v = in_run, f180 = false;
        uint8_t code = 0;
        uint64_t sc = 0;
        if (v) {
            if (a.rec) {
                const int32_t fl = a.rec[e].flags;
                v = (fl & 1) != 0;
                if (v) {
                    const float s = static_cast<float>(a.rec[e].prompt_i);
                    code = s < 0.0f ? 2 : (s > 0.0f ? 1 : 0);
                    sc = a.rec[e].sample_counter;
                    f180 = (fl & 4) != 0;
                }
            } else {
                if (a.valid) v = a.valid[e] != 0;
                if (v) {
                    const float s = a.sym[e];
                    code = s < 0.0f ? 2 : (s > 0.0f ? 1 : 0);
                    if (a.flags180) f180 = a.flags180[e] != 0;
                }
            }
        }
        const unsigned long long mask = __ballot(v);
        const int n = __popcll(mask);  // 0..64, wave-uniform
        const int ord = __popcll(mask & ((1ull << lane) - 1ull));
        uint32_t out_tow = 0;
        uint8_t out_sf = 0;
        if (n > 0) {
            if (size == 0) {  // seeding (:573-590), under the first symbol's 180° flag
                const bool inv = (__ballot(v && ord == 0 && f180)) != 0ull;
                if (lane < kLnavPre) {
                    const bool neg = (((inv ? kLnavPreOneMask : kLnavPreZeroMask) >> lane) & 1u) != 0;
                    buf[lane] = neg ? 2 : 1;
                }
                size = kLnavPre;
                counter += kLnavPre;
            }
            if (v) buf[size + ord] = code;  // size <= 300, ord < 64
            __syncthreads();

            // state-0 hits: after symbol `lane` the history is buf[o .. o + 300), o = size + lane + 1 − 300
            bool hit_match = false, hit_mismatch = false;
            if (lane < n && size + lane + 1 >= kLnavBits) {
                const int o = size + lane + 1 - kLnavBits;  // 0 <= o, o + 8 <= size
                uint32_t neg = 0;
                for (int i = 0; i < kLnavPre; i++) neg |= (buf[o + i] == 2 ? 1u : 0u) << i;
                hit_match = neg == kLnavPreZeroMask;
                hit_mismatch = neg == kLnavPreOneMask;
            }
            const unsigned long long mismatch = __ballot(hit_mismatch);
            const unsigned long long hits = __ballot(hit_match) | mismatch;

            int pos = 0;  // symbols [0, pos) of the chunk are done; `counter` is the block's after them
            while (pos < n) {
                int ev = n;  // the next symbol at which the machine does more than count
                if (stat == 0) {
                    const unsigned long long rest = pos < 64 ? hits & ~((1ull << pos) - 1ull) : 0ull;
                    if (rest) ev = __ffsll(rest) - 1;
                } else {
                    const uint64_t due = preamble_index + static_cast<uint64_t>(kLnavBits);
                    if (due <= counter + 1u) ev = pos;
                    else if (due - counter - 1u < static_cast<uint64_t>(n - pos)) ev = pos + static_cast<int>(due - counter - 1u);
                }
                if (ev > pos) {  // plain symbols pos .. ev − 1
                    if (stat == 0) tow_set = false;
                    if (v && ord >= pos && ord < ev) {
                        out_tow = tow_set ? tow_cur + 20u * static_cast<uint32_t>(ord - pos + 1) : tow_cur;
                        out_sf = (tow_set ? 1 : 0) | (pll180 ? 2 : 0);
                    }
                    if (tow_set) tow_cur += 20u * static_cast<uint32_t>(ev - pos);
                    counter += static_cast<uint64_t>(ev - pos);
                    pos = ev;
                }
                if (pos >= n) break;

                // ---- symbol `pos`: a state-0 hit, or a subframe is due ----
                counter += 1u;
                if (!sent && counter - last_valid > kLnavMaxWithoutValid) {  // check_tlm_separation, ahead of the machine
                    sent = true;
                    fault = true;
                }
                const bool was1 = stat == 1;
                preamble_index = counter;
                if (!was1) {
                    pll180 = ((mismatch >> pos) & 1ull) != 0;
                    prev_word = 0;
                }
                // decode_subframe over buf[o .. o + 300)
                tried += 1u;
                const int o = max(size + pos + 1 - kLnavBits, 0);  // o + 300 <= size + n <= 372
                uint32_t raw = 0;
                if (lane < 10) {
                    const uint8_t one = pll180 ? 2 : 1;
                    for (int b = 0; b < 30; b++) raw = (raw << 1) | (buf[o + 30 * lane + b] == one ? 1u : 0u);
                }
                uint32_t below = static_cast<uint32_t>(__shfl_up(static_cast<int>(raw), 1));
                if (lane == 0) below = prev_word;
                uint32_t word = raw | ((below & 1u) << 30) | ((below & 2u) << 30);
                if (word & 0x40000000u) word ^= 0x3FFFFFC0u;
                const uint32_t fail_mask = static_cast<uint32_t>(__ballot(lane < 10 && !lnav_parity(word)));
                prev_word = static_cast<uint32_t>(__shfl(static_cast<int>(word), 9));
                const uint32_t how = static_cast<uint32_t>(__shfl(static_cast<int>(word), 1));
                const int sid = static_cast<int>((how >> 8) & 7u);
                const bool ok = fail_mask == 0u && sid >= 1 && sid <= 5;
                if (ok) nav_tow = 6u * ((how >> 13) & 0x1FFFFu);

                bool lost = false;
                if (ok) {
                    crc_err = 0;
                    last_valid = counter;
                    frame_sync = true;
                    stat = 1;
                } else if (was1) {
                    crc_err++;
                    if (crc_err > kLnavCrcErrorLimit) {
                        frame_sync = false;
                        stat = 0;
                        tow_cur = tow_pre = 0;
                        crc_err = 0;
                        tow_set = false;
                        lost = true;
                    }
                }
                if (!was1) tow_set = false;  // state 0 ends so (:513)
                if (ok) {  // d_flag_preamble: the stamp (:605-617)
                    if (nav_tow != 0u) {
                        tow_cur = tow_pre = nav_tow * 1000u;
                        tow_set = true;
                    }
                } else if (tow_set) {
                    tow_cur += 20u;
                }
                if (v && ord == pos) {
                    out_tow = tow_cur;
                    out_sf = (tow_set ? 1 : 0) | (pll180 ? 2 : 0) | (ok ? 4 : 0);
                }
                if ((ok || was1) && count < a.subframes_per_run) {
                    // the completing entry's sample counter, from the lane that holds it
                    const unsigned long long holder = __ballot(v && ord == pos);
                    const int hl = holder ? __ffsll(holder) - 1 : 0;
                    const uint32_t sc_lo = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(sc)), hl));
                    const uint32_t sc_hi = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(sc >> 32)), hl));
                    gnsship_lnav_subframe* sf = a.subframes + (static_cast<size_t>(c) * a.subframes_per_run + count);
                    if (lane < 10) sf->words[lane] = word;
                    if (lane == 0) {
                        sf->symbol_counter = counter;
                        sf->sample_counter = a.rec ? (static_cast<uint64_t>(sc_hi) << 32) | sc_lo : 0ull;
                        sf->channel = c;
                        sf->subframe_id = sid;
                        sf->tow_s = nav_tow;
                        sf->crc_error_counter = crc_err;
                        sf->parity_fail_mask = fail_mask;
                        sf->flags = (ok ? 1 : 0) | (fail_mask == 0u ? 2 : 0) | (pll180 ? 4 : 0) | (was1 ? 8 : 0) | (frame_sync ? 16 : 0) | (lost ? 32 : 0);
                    }
                    count++;
                }
                pos++;
            }
            if (!sent && counter - last_valid > kLnavMaxWithoutValid) {
                sent = true;
                fault = true;
            }

            // the newest 300 entries move down to buf[0 .. 300)
            const int total = size + n, drop = max(total - kLnavBits, 0);
            if (drop > 0) {
                uint8_t keep[5];
                for (int j = 0; j < 5; j++) {
                    const int i = lane + 64 * j;  // < 320; i + drop < 320 + 72
                    keep[j] = i < kLnavBits ? buf[i + drop] : 0;
                }
                __syncthreads();
                for (int j = 0; j < 5; j++) {
                    const int i = lane + 64 * j;
                    if (i < kLnavBits) buf[i] = keep[j];
                }
            }
            size = total - drop;
            __syncthreads();
        }
        if (in_run) {
            a.tow_ms[e] = out_tow;
            a.sflags[e] = out_sf;
        }
    }

    tlm_codes_pack(buf, kLnavHistWords, cs->neg, cs->pos, size, lane);  // codes → the bit strings
    if (lane == 0) {
        gnsship_lnav_state o;
        o.symbol_counter = counter;
        o.preamble_index = preamble_index;
        o.last_valid_preamble = last_valid;
        o.subframes_tried = tried;
        o.prev_word = prev_word;
        o.tow_at_preamble_ms = tow_pre;
        o.tow_at_current_symbol_ms = tow_cur;
        o.nav_tow_s = nav_tow;
        o.stat = stat;
        o.crc_error_counter = crc_err;
        o.history_size = size;
        o.pll_180 = pll180;
        o.frame_sync = frame_sync;
        o.tow_set = tow_set;
        o.sent_tlm_failed = sent;
        cs->st = o;
        a.counts[c] = count;
        a.faults[c] = fault ? 1 : 0;
    }
}

// reset() (what 1) and set_satellite() (what 0) on one channel
__global__ void lnav_control_kernel(LnavChan* cs, int what)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (what) {
        cs->st.last_valid_preamble = cs->st.symbol_counter;
        cs->st.sent_tlm_failed = 0;
        cs->st.tow_set = 0;
        cs->st.history_size = 0;
        cs->st.stat = 0;
    } else {
        cs->st.nav_tow_s = 0;
    }
}

}  // namespace

struct gnsship_lnav {
    TlmHost h;  // h.mask: the 180° flags
    gnsship_lnav_conf conf = {};
    int32_t subframes_per_run = 0;
    LnavChan* chans_dev = nullptr;
    gnsship_lnav_subframe* subframes_dev = nullptr;
    int32_t* counts_dev = nullptr;
    uint8_t* faults_dev = nullptr;
    uint32_t* tow_dev = nullptr;
    uint8_t* sflags_dev = nullptr;
};

extern "C" int gnsship_lnav_destroy(gnsship_lnav* t)
{
    if (!t) return GNSSHIP_E_INVAL;
    t->h.release_all({t->chans_dev, t->subframes_dev, t->counts_dev, t->faults_dev, t->tow_dev, t->sflags_dev});
    delete t;
    return GNSSHIP_OK;
}

extern "C" int gnsship_lnav_create(gnsship_ctx* ctx, const gnsship_lnav_conf* conf, int32_t max_channels, gnsship_lnav** out)
{
    if (!ctx || !out) return GNSSHIP_E_INVAL;
    *out = nullptr;
    if (!conf) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_lnav_create: null configuration");
    if (conf->max_rounds < 1 || conf->max_rounds > GNSSHIP_LNAV_MAX_ROUNDS) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_lnav_create: 1 <= max_rounds <= 2^20");
    if (conf->reserved != 0) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_lnav_create: reserved must be 0");
    if (max_channels < 1 || max_channels > GNSSHIP_LNAV_MAX_CHANNELS) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_lnav_create: 1 <= max_channels <= 2^20");
    if (int rc = set_device(ctx)) return rc;
    gnsship_lnav* t = new (std::nothrow) gnsship_lnav();
    if (!t) return GNSSHIP_E_NOMEM;
    t->h.ctx = ctx;
    t->h.max_channels = max_channels;
    t->h.max_rounds = conf->max_rounds;
    t->conf = *conf;
    t->subframes_per_run = GNSSHIP_LNAV_SUBFRAMES_PER_RUN(conf->max_rounds);
    const size_t nc = static_cast<size_t>(max_channels), slots = nc * t->subframes_per_run, entries = nc * conf->max_rounds;
    const hipError_t e = alloc_all(ctx, {dev_alloc(&t->chans_dev, nc, true), dev_alloc(&t->subframes_dev, slots, true), dev_alloc(&t->counts_dev, nc, true),
                                            dev_alloc(&t->faults_dev, nc, true), dev_alloc(&t->tow_dev, entries, true), dev_alloc(&t->sflags_dev, entries, true)});
    if (e != hipSuccess) {
        gnsship_lnav_destroy(t);
        return hip_fail(ctx, e, "gnsship_lnav_create");
    }
    *out = t;
    return GNSSHIP_OK;
}

// Launch over n_rounds entries per channel already on the device, then copy what the caller wants.
static int lnav_launch(gnsship_lnav* t, const float* sym, const uint8_t* valid, const uint8_t* flags180, const gnsship_trk_epoch* rec, int32_t n_rounds,
    gnsship_lnav_subframe* subframes_host, int32_t* counts_host, uint8_t* faults_host, uint32_t* tow_ms_host, uint8_t* sflags_host, const char* who)
{
    gnsship_ctx* ctx = t->h.ctx;
    LnavArgs a = {};
    a.sym = sym;
    a.valid = valid;
    a.flags180 = flags180;
    a.rec = rec;
    a.chans = t->chans_dev;
    a.subframes = t->subframes_dev;
    a.counts = t->counts_dev;
    a.faults = t->faults_dev;
    a.tow_ms = t->tow_dev;
    a.sflags = t->sflags_dev;
    a.max_channels = t->h.max_channels;
    a.n_rounds = n_rounds;
    a.subframes_per_run = t->subframes_per_run;
    hipLaunchKernelGGL(lnav_kernel, dim3(static_cast<unsigned>(t->h.max_channels)), dim3(64), 0, ctx->stream, a);
    if (int rc = launched(ctx, who)) return rc;
    const size_t nc = static_cast<size_t>(t->h.max_channels), slots = nc * t->subframes_per_run, entries = nc * n_rounds;
    return copy_out(ctx, {{subframes_host, t->subframes_dev, sizeof(gnsship_lnav_subframe) * slots}, {counts_host, t->counts_dev, sizeof(int32_t) * nc},
                                 {faults_host, t->faults_dev, nc}, {tow_ms_host, t->tow_dev, sizeof(uint32_t) * entries}, {sflags_host, t->sflags_dev, entries}}, who);
}

extern "C" int gnsship_lnav_run_symbols(gnsship_lnav* t, const float* symbols, const uint8_t* valid, const uint8_t* flags180, int on_device,
    int32_t n_rounds, gnsship_lnav_subframe* subframes_host, int32_t* counts_host, uint8_t* faults_host, uint32_t* tow_ms_host, uint8_t* sflags_host)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_lnav_run_symbols";
    if (int rc = tlm_symbols_in(t->h, who, on_device, n_rounds, &symbols, &valid, &flags180)) return rc;
    return lnav_launch(t, symbols, valid, flags180, nullptr, n_rounds, subframes_host, counts_host, faults_host, tow_ms_host, sflags_host, who);
}

extern "C" int gnsship_lnav_run_records(gnsship_lnav* t, const gnsship_trk_epoch* records, int on_device, int32_t n_rounds,
    gnsship_lnav_subframe* subframes_host, int32_t* counts_host, uint8_t* faults_host, uint32_t* tow_ms_host, uint8_t* sflags_host)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_lnav_run_records";
    if (int rc = tlm_records_in(t->h, who, on_device, n_rounds, &records)) return rc;
    return lnav_launch(t, nullptr, nullptr, nullptr, records, n_rounds, subframes_host, counts_host, faults_host, tow_ms_host, sflags_host, who);
}

extern "C" int gnsship_lnav_run_trk(gnsship_lnav* t, gnsship_trk* trk, gnsship_lnav_subframe* subframes_host, int32_t* counts_host, uint8_t* faults_host,
    uint32_t* tow_ms_host, uint8_t* sflags_host, int32_t* n_rounds_out)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_lnav_run_trk";
    const gnsship_trk_epoch* rec = nullptr;
    int32_t rounds = 0;
    if (int rc = tlm_trk_in(t->h, who, trk, &rec, &rounds)) return rc;
    if (n_rounds_out) *n_rounds_out = rounds;
    return lnav_launch(t, nullptr, nullptr, nullptr, rec, rounds, subframes_host, counts_host, faults_host, tow_ms_host, sflags_host, who);
}

extern "C" int gnsship_lnav_outputs_device(gnsship_lnav* t, gnsship_lnav_subframe** subframes, int32_t** counts, uint8_t** faults, uint32_t** tow_ms,
    uint8_t** sflags, int32_t* subframes_per_run)
{
    if (!t) return GNSSHIP_E_INVAL;
    if (subframes) *subframes = t->subframes_dev;
    if (counts) *counts = t->counts_dev;
    if (faults) *faults = t->faults_dev;
    if (tow_ms) *tow_ms = t->tow_dev;
    if (sflags) *sflags = t->sflags_dev;
    if (subframes_per_run) *subframes_per_run = t->subframes_per_run;
    return GNSSHIP_OK;
}

static int lnav_control(gnsship_lnav* t, int32_t channel, int what, const char* who)
{
    if (!t) return GNSSHIP_E_INVAL;
    if (int rc = tlm_check_channel(t->h, who, channel)) return rc;
    if (int rc = set_device(t->h.ctx)) return rc;
    hipLaunchKernelGGL(lnav_control_kernel, dim3(1), dim3(1), 0, t->h.ctx->stream, t->chans_dev + channel, what);
    return launched(t->h.ctx, who);
}

extern "C" int gnsship_lnav_reset_channel(gnsship_lnav* t, int32_t channel) { return lnav_control(t, channel, 1, "gnsship_lnav_reset_channel"); }

extern "C" int gnsship_lnav_set_satellite(gnsship_lnav* t, int32_t channel) { return lnav_control(t, channel, 0, "gnsship_lnav_set_satellite"); }

extern "C" int gnsship_lnav_new_channel(gnsship_lnav* t, int32_t channel)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_lnav_new_channel";
    if (int rc = tlm_check_channel(t->h, who, channel)) return rc;
    if (int rc = set_device(t->h.ctx)) return rc;
    const hipError_t e = hipMemsetAsync(t->chans_dev + channel, 0, sizeof(LnavChan), t->h.ctx->stream);
    return e == hipSuccess ? GNSSHIP_OK : hip_fail(t->h.ctx, e, who);
}

extern "C" int gnsship_lnav_state_get(gnsship_lnav* t, int32_t channel, gnsship_lnav_state* st)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_lnav_state_get";
    if (int rc = tlm_check_state(t->h, who, channel, st)) return rc;
    if (int rc = set_device(t->h.ctx)) return rc;
    return copy_out(t->h.ctx, {{st, &t->chans_dev[channel].st, sizeof(*st)}}, who);
}
