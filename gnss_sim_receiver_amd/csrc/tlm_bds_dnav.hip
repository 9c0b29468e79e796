// tlm_bds_dnav.hip — beidou_b1i_telemetry_decoder_gs and beidou_b3i_telemetry_decoder_gs on the device up to the time of
// week (include/gnsship.h, gnsship_dnav_*): the 311-symbol history, the 11-symbol preamble correlation, the three-state
// frame synchronisation, decode_subframe with the de-interleaver and decode_bch15_11_01, the FraID / Pnum / SOW logic of
// d1_subframe_decoder and d2_subframe_decoder, and the TOW stamp of every symbol.  One kernel, the signal a mode: the two
// blocks differ only in which PRNs take the D2 decoder.  Input: floats with a validity mask and output-valid flags, or
// tracking's epoch records (host, device, or in place where gnsship_trk left them).  Output: one record per decode and
// the block's output stream (tow_ms, sflags) per entry.
//
// Layout: one workgroup of one wavefront per channel, as tlm_gps_lnav.hip and for its reason.  No float arithmetic: the
// block only ever asks `x < 0` and `x > 0` of a symbol, so an entry is one of three codes — 0 (zero, −0, NaN: both tests
// false), 1 (> 0), 2 (< 0) — and NaN and ±0 behave exactly as in the block (negating a float exchanges codes 1 and 2).
//   history  in HBM two 311-bit strings per channel (neg, pos; bit i is the i-th oldest entry), 80 bytes.  For the run
//            they are unpacked into a linear LDS buffer of codes, oldest first, and packed again once at the end
//            (tlm_device.h, shared with tlm_gps_lnav.hip).
//   gather   64 entries at a time; a ballot of the valid entries and a prefix popcount give each symbol its ordinal, and
//            the chunk's n symbols are appended at buf[size .. size + n).  The history after the chunk's k-th symbol is the
//            311 entries ending at buf[size + k].  After the chunk the newest 311 entries move down.
//   hits     lane k forms the "< 0" pattern of the 11 oldest entries as they stand after the chunk's k-th symbol, when
//            there are 311; corr = 11 − 2 · (bits that differ from the preamble's zeros).  Two ballots give the hits.
//   machine  wave-uniform: states 0 and 1 walk the hit ballot with find-first-set, state 2 jumps to the due symbol
//            (counter == preamble_index + 300).  Between two such symbols only the TOW moves.
//   decode   lane 0 takes word 1; lanes 1..18 each take one BCH row (word 2 + (lane − 1) / 2, row (lane − 1) & 1): 15 codes to
//            bits under the polarity, the syndrome as four masked parities (the ±1 shift register of the source is linear
//            over GF(2): mask k is the set of input positions that reach reg[k]), one bit flipped through errind.  Lanes
//            1..9 then join two rows to a word by shuffle.
//   outputs  every lane keeps the tow_ms / sflags of its own entry; between decodes valid_word's TOW is base + d · (distance),
//            up to and including the first entry whose output-valid flag is false.
// Every LDS and HBM index comes from lane numbers, sizes and ballot bits, never from a symbol's value.
// The host path around the kernel (staging, the run calls' checks, output copies) is tlm_host.h.
#include <new>

#include "tlm_device.h"
#include "tlm_host.h"

using namespace gnsship;

namespace {

constexpr int kDnavPeriod = 300;              // BEIDOU_DNAV_PREAMBLE_PERIOD_SYMBOLS, BEIDOU_DNAV_SUBFRAME_SYMBOLS
constexpr int kDnavPre = 11;                  // BEIDOU_DNAV_PREAMBLE_LENGTH_SYMBOLS
constexpr int kDnavRequired = 311;            // d_required_symbols, the history's capacity
constexpr uint32_t kDnavPreOneMask = 0x247u;  // "11100010010": bit i set where preamble[i] is '1'
constexpr uint32_t kDnavPreZeroMask = 0x5B8u;
constexpr uint32_t kDnavLeap = 14;            // BEIDOU_DNAV_BDT2GPST_LEAP_SEC_OFFSET
constexpr int kDnavBuf = 384;                 // 311 + 64 appended = 375, rounded up
constexpr int kDnavHistWords = 10;            // 320 bits hold 311

struct DnavChan {  // one block object's members
    gnsship_dnav_state st;
    uint32_t neg[kDnavHistWords], pos[kDnavHistWords];
};
static_assert(sizeof(DnavChan) == 144, "DnavChan");

struct DnavArgs {
    const float* sym;              // n_rounds × max_channels, or null
    const uint8_t* valid;          // the same shape, or null
    const uint8_t* out_valid;      // the same shape, or null
    const gnsship_trk_epoch* rec;  // the same shape, or null (then sym)
    DnavChan* chans;
    gnsship_dnav_subframe* subframes;  // max_channels × subframes_per_run
    int32_t* counts;
    uint32_t* tow_ms;              // max_rounds × max_channels
    uint8_t* sflags;               // the same shape
    int32_t max_channels, n_rounds, subframes_per_run;
};

// decode_bch15_11_01 on a row of 15 bits (bit 14 is bits[0], 1 is +1): the corrected row, and whether the syndrome was non-zero
__device__ __forceinline__ uint32_t dnav_bch(uint32_t row, bool* touched)
{
    const uint32_t err = (__popc(row & 0x7591u) & 1) | ((__popc(row & 0x1EB2u) & 1) << 1) | ((__popc(row & 0x3D64u) & 1) << 2) |
        ((__popc(row & 0x7AC8u) & 1) << 3);
    // errind {14, 13, 10, 12, 6, 9, 4, 11, 0, 5, 7, 8, 1, 3, 2}, four bits each, entry err − 1
    const uint64_t errind = 0x2318750B496CADEull;
    *touched = err != 0u;
    if (err != 0u) row ^= 1u << (14 - static_cast<int>((errind >> (4 * (err - 1u))) & 0xFull));
    return row;
}

__global__ __launch_bounds__(64) void dnav_kernel(const DnavArgs a)
{
    __shared__ uint8_t buf[kDnavBuf];
    __shared__ uint8_t ovs[64];  // the chunk's output-valid flags by ordinal
    const int lane = threadIdx.x;
    const int c = blockIdx.x;  // the grid is max_channels workgroups

    DnavChan* cs = a.chans + c;
    uint64_t counter = tlm_uniform64(cs->st.symbol_counter), preamble_index = tlm_uniform64(cs->st.preamble_index);
    uint64_t last_valid = tlm_uniform64(cs->st.last_valid_preamble);
    uint32_t tow_pre = tlm_uniform(cs->st.tow_at_preamble_ms), tow_cur = tlm_uniform(cs->st.tow_at_current_symbol_ms);
    uint32_t sow = tlm_uniform(cs->st.sow);
    const uint32_t d = tlm_uniform(static_cast<int>(cs->st.d2_timing)) != 0 ? 2u : 20u;
    const bool d2 = tlm_uniform(static_cast<int>(cs->st.d2_decoder)) != 0;
    int stat = min(max(tlm_uniform(cs->st.stat), 0), 2);
    int size = min(max(tlm_uniform(cs->st.history_size), 0), kDnavRequired);
    bool sow_set = tlm_uniform(static_cast<int>(cs->st.sow_set)) != 0, frame_sync = tlm_uniform(static_cast<int>(cs->st.frame_sync)) != 0;
    bool valid_word = tlm_uniform(static_cast<int>(cs->st.valid_word)) != 0;
    bool new_sow = tlm_uniform(static_cast<int>(cs->st.new_sow_available)) != 0;

    tlm_codes_unpack(buf, kDnavBuf, cs->neg, cs->pos, size, lane);  // the bit strings → codes, oldest first
    __syncthreads();

    int count = 0;
    for (int base = 0; base < a.n_rounds; base += 64) {
        const int r = base + lane;
        const bool in_run = r < a.n_rounds;
        const size_t e = static_cast<size_t>(in_run ? r : 0) * a.max_channels + c;
        bool v = in_run, ov = true;
        uint8_t code = 0;
        uint64_t sc = 0;
        if (v) {
            if (a.rec) {
                v = (a.rec[e].flags & 1) != 0;
                if (v) {
                    const float s = static_cast<float>(a.rec[e].prompt_i);
                    code = s < 0.0f ? 2 : (s > 0.0f ? 1 : 0);
                    sc = a.rec[e].sample_counter;
                }
            } else {
                if (a.valid) v = a.valid[e] != 0;
                if (v) {
                    const float s = a.sym[e];
                    code = s < 0.0f ? 2 : (s > 0.0f ? 1 : 0);
                    if (a.out_valid) ov = a.out_valid[e] != 0;
                }
            }
        }
        const unsigned long long mask = __ballot(v);
        const int n = __popcll(mask);  // 0..64, wave-uniform
        const int ord = __popcll(mask & ((1ull << lane) - 1ull));
        uint32_t out_tow = 0;
        uint8_t out_sf = 0;
        if (n > 0) {
            if (v) {
                buf[size + ord] = code;  // size <= 311, ord < 64
                ovs[ord] = ov ? 1 : 0;
            }
            __syncthreads();

            // after symbol `lane` the history is buf[o .. o + 311), o = size + lane + 1 − 311, once it holds 311
            bool full = false;
            uint32_t differ = 0;  // among the 11 oldest, the entries whose "< 0" is not the preamble's
            if (lane < n && size + lane + 1 >= kDnavRequired) {
                const int o = size + lane + 1 - kDnavRequired;  // 0 <= o, o + 11 <= size + lane + 1
                uint32_t neg = 0;
                for (int i = 0; i < kDnavPre; i++) neg |= (buf[o + i] == 2 ? 1u : 0u) << i;
                differ = neg ^ kDnavPreZeroMask;
                full = true;
            }
            // corr = 11 − 2 · popcount(differ): +11 when nothing differs, −11 when everything does
            const unsigned long long hits = __ballot(full && (differ == 0u || differ == 0x7FFu));
            const unsigned long long normal = __ballot(full && __popc(differ) <= 5);  // corr > 0
            const unsigned long long drops = __ballot(lane < n && ovs[lane] == 0);    // by ordinal

            int pos = 0;  // symbols [0, pos) of the chunk are done; `counter` is the block's after them
            while (pos < n) {
                int ev = n;  // the next symbol at which the machine does more than count
                if (stat != 2) {
                    const unsigned long long rest = hits & ~((1ull << pos) - 1ull);  // pos < n <= 64
                    if (rest) ev = __ffsll(rest) - 1;
                } else {
                    const uint64_t due = preamble_index + static_cast<uint64_t>(kDnavPeriod);
                    if (due > counter && due - counter - 1u < static_cast<uint64_t>(n - pos)) ev = pos + static_cast<int>(due - counter - 1u);
                }
                bool decode = false, state1 = false;
                int last = ev;  // plain symbols run to here (exclusive): an event without a stamp is plain for the TOW
                if (ev < n) {
                    const uint64_t at = counter + static_cast<uint64_t>(ev - pos) + 1u;  // the counter at the event
                    if (stat == 0) {
                        preamble_index = at;
                        stat = 1;
                    } else if (stat == 1) {
                        const int32_t diff = static_cast<int32_t>(at - preamble_index);
                        if (diff == kDnavPeriod) {
                            decode = state1 = true;
                            stat = 2;
                        } else if (diff > kDnavPeriod) {
                            stat = 0;
                        }
                    } else {
                        decode = true;
                    }
                    if (!decode) last = ev + 1;
                }

                uint32_t word = 0, fra_id = 0, pnum = 0, corrected = 0;
                bool inverted = false, stamped = false;
                if (decode) {  // decode_subframe over buf[o .. o + 300), the 300 oldest
                    const int o = max(size + ev + 1 - kDnavRequired, 0);  // o + 300 <= size + n
                    inverted = ((normal >> ev) & 1ull) == 0ull;
                    const uint8_t one = inverted ? 2 : 1;
                    uint32_t row = 0;
                    bool touched = false;
                    if (lane == 0) {
                        for (int b = 0; b < 30; b++) row = (row << 1) | (buf[o + b] == one ? 1u : 0u);
                    } else if (lane <= 18) {
                        const int w = 1 + ((lane - 1) >> 1), rr = (lane - 1) & 1;
                        for (int b = 0; b < 15; b++) row = (row << 1) | (buf[o + 30 * w + 2 * b + rr] == one ? 1u : 0u);
                        row = dnav_bch(row, &touched);
                    }
                    corrected = static_cast<uint32_t>(__ballot(touched) >> 1);
                    const int src = lane >= 1 && lane <= 9 ? 2 * lane - 1 : 0;
                    const uint32_t ra = static_cast<uint32_t>(__shfl(static_cast<int>(row), src));
                    const uint32_t rb = static_cast<uint32_t>(__shfl(static_cast<int>(row), src + 1));
                    word = lane == 0 ? row : ((ra >> 4) << 19) | ((rb >> 4) << 8) | ((ra & 0xFu) << 4) | (rb & 0xFu);
                    const uint32_t w0 = static_cast<uint32_t>(__shfl(static_cast<int>(word), 0));
                    const uint32_t w1 = static_cast<uint32_t>(__shfl(static_cast<int>(word), 1));
                    fra_id = (w0 >> 12) & 7u;                                   // bits 16..18
                    pnum = d2 ? (w1 >> 14) & 0xFu : (w1 >> 10) & 0x7Fu;         // bits 43..46, bits 44..50
                    const bool takes = d2 ? fra_id == 1u && pnum >= 1u && pnum <= 10u : fra_id >= 1u && fra_id <= 5u;
                    if (takes) {
                        sow = (((w0 >> 4) & 0xFFu) << 12) | ((w1 >> 18) & 0xFFFu);  // bits 19..26 ‖ 31..42
                        new_sow = true;
                    }
                    frame_sync = true;
                    stamped = new_sow;
                }

                // plain symbols pos .. last − 1
                if (last > pos) {
                    int adds = 0;  // how many of them move the TOW
                    bool falls = false;
                    if (valid_word) {
                        const unsigned long long dr = drops & ~((1ull << pos) - 1ull) & (last < 64 ? (1ull << last) - 1ull : ~0ull);
                        adds = dr ? __ffsll(dr) - pos : last - pos;
                        falls = dr != 0ull;
                    }
                    if (v && ord >= pos && ord < last) {
                        const int k = ord - pos + 1;
                        out_tow = tow_cur + d * static_cast<uint32_t>(min(k, adds));
                        out_sf = valid_word && !(falls && k >= adds) ? GNSSHIP_DNAV_S_VALID_WORD : 0;
                    }
                    tow_cur += d * static_cast<uint32_t>(adds);
                    if (falls) valid_word = false;
                }
                counter += static_cast<uint64_t>(min(ev + 1, n) - pos);
                if (decode) {
                    preamble_index = counter;
                    bool zeroed = false;
                    if (stamped) {  // :629-663
                        tow_pre = (sow + kDnavLeap) * 1000u;
                        const uint32_t before = tow_cur;
                        tow_cur = tow_pre + static_cast<uint32_t>(kDnavRequired) * d;
                        sow_set = true;
                        new_sow = false;
                        const int64_t delta = static_cast<int64_t>(tow_cur) - static_cast<int64_t>(before);
                        if (before != 0u && (delta < 0 ? -delta : delta) > static_cast<int64_t>(d)) {
                            tow_cur = 0;
                            valid_word = false;
                            zeroed = true;
                        } else {
                            last_valid = counter;
                            valid_word = true;
                        }
                    } else if (valid_word) {  // :664-674
                        tow_cur += d;
                        if (((drops >> ev) & 1ull) != 0ull) valid_word = false;
                    }
                    if (v && ord == ev) {
                        out_tow = tow_cur;
                        out_sf = (valid_word ? GNSSHIP_DNAV_S_VALID_WORD : 0) | GNSSHIP_DNAV_S_SUBFRAME | (inverted ? GNSSHIP_DNAV_S_INVERTED : 0);
                    }
                    if (count < a.subframes_per_run) {
                        // the completing entry's sample counter, from the lane that holds it
                        const unsigned long long holder = __ballot(v && ord == ev);
                        const int hl = holder ? __ffsll(holder) - 1 : 0;
                        const uint32_t sc_lo = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(sc)), hl));
                        const uint32_t sc_hi = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(sc >> 32)), hl));
                        gnsship_dnav_subframe* sf = a.subframes + (static_cast<size_t>(c) * a.subframes_per_run + count);
                        if (lane < 10) sf->words[lane] = word;
                        if (lane == 0) {
                            sf->symbol_counter = counter;
                            sf->sample_counter = a.rec ? (static_cast<uint64_t>(sc_hi) << 32) | sc_lo : 0ull;
                            sf->channel = c;
                            sf->fra_id = static_cast<int32_t>(fra_id);
                            sf->pnum = static_cast<int32_t>(pnum);
                            sf->sow = sow;
                            sf->corrected_mask = corrected;
                            sf->tow_at_current_symbol_ms = tow_cur;
                            sf->flags = (inverted ? GNSSHIP_DNAV_INVERTED : 0) | (state1 ? GNSSHIP_DNAV_STATE1 : 0) | (stamped ? GNSSHIP_DNAV_NEW_SOW : 0) |
                                (d2 ? GNSSHIP_DNAV_D2_DECODER : 0) | (d == 2u ? GNSSHIP_DNAV_D2_TIMING : 0) | (zeroed ? GNSSHIP_DNAV_TOW_ZEROED : 0);
                            sf->reserved = 0;
                        }
                        count++;
                    }
                }
                pos = min(ev + 1, n);
            }

            // the newest 311 entries move down to buf[0 .. 311)
            const int total = size + n, drop = max(total - kDnavRequired, 0);
            if (drop > 0) {
                uint8_t keep[5];
                for (int j = 0; j < 5; j++) {
                    const int i = lane + 64 * j;  // < 320; i + drop < 311 + 64
                    keep[j] = i < kDnavRequired ? buf[i + drop] : 0;
                }
                __syncthreads();
                for (int j = 0; j < 5; j++) {
                    const int i = lane + 64 * j;
                    if (i < kDnavRequired) buf[i] = keep[j];
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

    tlm_codes_pack(buf, kDnavHistWords, cs->neg, cs->pos, size, lane);  // codes → the bit strings
    if (lane == 0) {
        gnsship_dnav_state o = cs->st;  // prn, symbol_duration_ms, the decoder choice, sent_tlm_failed: as they were
        o.symbol_counter = counter;
        o.preamble_index = preamble_index;
        o.last_valid_preamble = last_valid;
        o.tow_at_preamble_ms = tow_pre;
        o.tow_at_current_symbol_ms = tow_cur;
        o.sow = sow;
        o.stat = stat;
        o.crc_error_counter = 0;
        o.history_size = size;
        o.sow_set = sow_set;
        o.frame_sync = frame_sync;
        o.valid_word = valid_word;
        o.new_sow_available = new_sow;
        cs->st = o;
        a.counts[c] = count;
    }
}

// what 0: reset(); 1: set_satellite(prn); 2: a new object on prn.  One thread per channel of [first, first + n).
__global__ void dnav_control_kernel(DnavChan* chans, int first, int n, int what, int prn, int signal)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DnavChan* cs = chans + first + i;
    if (what == 0) {
        cs->st.last_valid_preamble = cs->st.symbol_counter;
        cs->st.tow_at_current_symbol_ms = 0;
        cs->st.sent_tlm_failed = 0;
        cs->st.valid_word = 0;
        return;
    }
    if (what == 2) {
        gnsship_dnav_state z = {};
        cs->st = z;
        for (int w = 0; w < kDnavHistWords; w++) cs->neg[w] = cs->pos[w] = 0;
    }
    const bool geo = (prn > 0 && prn < 6) || prn > 58;
    cs->st.prn = prn;
    cs->st.d2_timing = geo ? 1 : 0;
    cs->st.symbol_duration_ms = geo ? 2u : 20u;
    cs->st.d2_decoder = (signal == GNSSHIP_DNAV_B1I ? geo : (prn > 0 && prn < 6)) ? 1 : 0;
}

}  // namespace

struct gnsship_dnav {
    TlmHost h;  // h.mask: the output-valid flags
    gnsship_dnav_conf conf = {};
    int32_t subframes_per_run = 0;
    DnavChan* chans_dev = nullptr;
    gnsship_dnav_subframe* subframes_dev = nullptr;
    int32_t* counts_dev = nullptr;
    uint32_t* tow_dev = nullptr;
    uint8_t* sflags_dev = nullptr;
};

extern "C" int gnsship_dnav_destroy(gnsship_dnav* t)
{
    if (!t) return GNSSHIP_E_INVAL;
    t->h.release_all({t->chans_dev, t->subframes_dev, t->counts_dev, t->tow_dev, t->sflags_dev});
    delete t;
    return GNSSHIP_OK;
}

static int dnav_control(gnsship_dnav* t, int first, int n, int what, int prn, const char* who)
{
    hipLaunchKernelGGL(dnav_control_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, t->h.ctx->stream, t->chans_dev, first, n, what, prn,
        t->conf.signal);
    return launched(t->h.ctx, who);
}

extern "C" int gnsship_dnav_create(gnsship_ctx* ctx, const gnsship_dnav_conf* conf, int32_t max_channels, gnsship_dnav** out)
{
    if (!ctx || !out) return GNSSHIP_E_INVAL;
    *out = nullptr;
    if (!conf) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_dnav_create: null configuration");
    if (conf->max_rounds < 1 || conf->max_rounds > GNSSHIP_DNAV_MAX_ROUNDS) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_dnav_create: 1 <= max_rounds <= 2^20");
    if (conf->signal != GNSSHIP_DNAV_B1I && conf->signal != GNSSHIP_DNAV_B3I)
        return fail(ctx, GNSSHIP_E_INVAL, "gnsship_dnav_create: signal must be GNSSHIP_DNAV_B1I or GNSSHIP_DNAV_B3I");
    if (conf->reserved != 0) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_dnav_create: reserved must be 0");
    if (max_channels < 1 || max_channels > GNSSHIP_DNAV_MAX_CHANNELS) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_dnav_create: 1 <= max_channels <= 2^20");
    if (int rc = set_device(ctx)) return rc;
    gnsship_dnav* t = new (std::nothrow) gnsship_dnav();
    if (!t) return GNSSHIP_E_NOMEM;
    t->h.ctx = ctx;
    t->h.max_channels = max_channels;
    t->h.max_rounds = conf->max_rounds;
    t->conf = *conf;
    t->subframes_per_run = GNSSHIP_DNAV_SUBFRAMES_PER_RUN(conf->max_rounds);
    const size_t nc = static_cast<size_t>(max_channels), slots = nc * t->subframes_per_run, entries = nc * conf->max_rounds;
    const hipError_t e = alloc_all(ctx, {dev_alloc(&t->chans_dev, nc, false), dev_alloc(&t->subframes_dev, slots, true), dev_alloc(&t->counts_dev, nc, true),
                                            dev_alloc(&t->tow_dev, entries, true), dev_alloc(&t->sflags_dev, entries, true)});
    if (e != hipSuccess) {
        gnsship_dnav_destroy(t);
        return hip_fail(ctx, e, "gnsship_dnav_create");
    }
    if (int rc = dnav_control(t, 0, max_channels, 2, 0, "gnsship_dnav_create")) {  // every channel a new object on PRN 0
        gnsship_dnav_destroy(t);
        return rc;
    }
    *out = t;
    return GNSSHIP_OK;
}

// Launch over n_rounds entries per channel already on the device, then copy what the caller wants.
static int dnav_launch(gnsship_dnav* t, const float* sym, const uint8_t* valid, const uint8_t* out_valid, const gnsship_trk_epoch* rec, int32_t n_rounds,
    gnsship_dnav_subframe* subframes_host, int32_t* counts_host, uint32_t* tow_ms_host, uint8_t* sflags_host, const char* who)
{
    gnsship_ctx* ctx = t->h.ctx;
    DnavArgs a = {};
    a.sym = sym;
    a.valid = valid;
    a.out_valid = out_valid;
    a.rec = rec;
    a.chans = t->chans_dev;
    a.subframes = t->subframes_dev;
    a.counts = t->counts_dev;
    a.tow_ms = t->tow_dev;
    a.sflags = t->sflags_dev;
    a.max_channels = t->h.max_channels;
    a.n_rounds = n_rounds;
    a.subframes_per_run = t->subframes_per_run;
    hipLaunchKernelGGL(dnav_kernel, dim3(static_cast<unsigned>(t->h.max_channels)), dim3(64), 0, ctx->stream, a);
    if (int rc = launched(ctx, who)) return rc;
    const size_t nc = static_cast<size_t>(t->h.max_channels), slots = nc * t->subframes_per_run, entries = nc * n_rounds;
    return copy_out(ctx, {{subframes_host, t->subframes_dev, sizeof(gnsship_dnav_subframe) * slots}, {counts_host, t->counts_dev, sizeof(int32_t) * nc},
                                 {tow_ms_host, t->tow_dev, sizeof(uint32_t) * entries}, {sflags_host, t->sflags_dev, entries}}, who);
}

extern "C" int gnsship_dnav_run_symbols(gnsship_dnav* t, const float* symbols, const uint8_t* valid, const uint8_t* out_valid, int on_device,
    int32_t n_rounds, gnsship_dnav_subframe* subframes_host, int32_t* counts_host, uint32_t* tow_ms_host, uint8_t* sflags_host)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_dnav_run_symbols";
    if (int rc = tlm_symbols_in(t->h, who, on_device, n_rounds, &symbols, &valid, &out_valid)) return rc;
    return dnav_launch(t, symbols, valid, out_valid, nullptr, n_rounds, subframes_host, counts_host, tow_ms_host, sflags_host, who);
}

extern "C" int gnsship_dnav_run_records(gnsship_dnav* t, const gnsship_trk_epoch* records, int on_device, int32_t n_rounds,
    gnsship_dnav_subframe* subframes_host, int32_t* counts_host, uint32_t* tow_ms_host, uint8_t* sflags_host)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_dnav_run_records";
    if (int rc = tlm_records_in(t->h, who, on_device, n_rounds, &records)) return rc;
    return dnav_launch(t, nullptr, nullptr, nullptr, records, n_rounds, subframes_host, counts_host, tow_ms_host, sflags_host, who);
}

extern "C" int gnsship_dnav_run_trk(gnsship_dnav* t, gnsship_trk* trk, gnsship_dnav_subframe* subframes_host, int32_t* counts_host,
    uint32_t* tow_ms_host, uint8_t* sflags_host, int32_t* n_rounds_out)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_dnav_run_trk";
    const gnsship_trk_epoch* rec = nullptr;
    int32_t rounds = 0;
    if (int rc = tlm_trk_in(t->h, who, trk, &rec, &rounds)) return rc;
    if (n_rounds_out) *n_rounds_out = rounds;
    return dnav_launch(t, nullptr, nullptr, nullptr, rec, rounds, subframes_host, counts_host, tow_ms_host, sflags_host, who);
}

extern "C" int gnsship_dnav_outputs_device(gnsship_dnav* t, gnsship_dnav_subframe** subframes, int32_t** counts, uint32_t** tow_ms, uint8_t** sflags,
    int32_t* subframes_per_run)
{
    if (!t) return GNSSHIP_E_INVAL;
    if (subframes) *subframes = t->subframes_dev;
    if (counts) *counts = t->counts_dev;
    if (tow_ms) *tow_ms = t->tow_dev;
    if (sflags) *sflags = t->sflags_dev;
    if (subframes_per_run) *subframes_per_run = t->subframes_per_run;
    return GNSSHIP_OK;
}

// reset_channel (what 0, PRN 0), set_satellite (1) and new_channel (2) on one channel
static int dnav_channel_call(gnsship_dnav* t, int32_t channel, int what, int32_t prn, const char* who)
{
    if (!t) return GNSSHIP_E_INVAL;
    if (int rc = tlm_check_channel(t->h, who, channel)) return rc;
    if (prn < 0 || prn > 63) return reject(t->h.ctx, GNSSHIP_E_INVAL, who, "0 <= prn <= 63");
    if (int rc = set_device(t->h.ctx)) return rc;
    return dnav_control(t, channel, 1, what, prn, who);
}

extern "C" int gnsship_dnav_reset_channel(gnsship_dnav* t, int32_t channel) { return dnav_channel_call(t, channel, 0, 0, "gnsship_dnav_reset_channel"); }

extern "C" int gnsship_dnav_set_satellite(gnsship_dnav* t, int32_t channel, int32_t prn)
{
    return dnav_channel_call(t, channel, 1, prn, "gnsship_dnav_set_satellite");
}

extern "C" int gnsship_dnav_new_channel(gnsship_dnav* t, int32_t channel, int32_t prn)
{
    return dnav_channel_call(t, channel, 2, prn, "gnsship_dnav_new_channel");
}

extern "C" int gnsship_dnav_state_get(gnsship_dnav* t, int32_t channel, gnsship_dnav_state* st)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_dnav_state_get";
    if (int rc = tlm_check_state(t->h, who, channel, st)) return rc;
    if (int rc = set_device(t->h.ctx)) return rc;
    return copy_out(t->h.ctx, {{st, &t->chans_dev[channel].st, sizeof(*st)}}, who);
}
