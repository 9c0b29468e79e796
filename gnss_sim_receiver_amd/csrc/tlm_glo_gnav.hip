// tlm_glo_gnav.hip — glonass_l1_ca_telemetry_decoder_gs and glonass_l2_ca_telemetry_decoder_gs on the device up to the time
// of week (include/gnsship.h, gnsship_gnav_*): the 2000-symbol history, the 300-symbol time-mark correlation over its oldest
// entries, the three-state frame synchronisation, decode_string with its double half-bit sums, CRC_test, what string_decoder
// keeps of strings 1..5, have_new_ephemeris / have_new_utc_model, glot_to_gpst and the TOW stamp of every symbol.  One
// kernel serves both blocks.  Input: floats with a validity mask, or tracking's epoch records (host, device, or in place
// where gnsship_trk left them).  Output: one record per decode and the block's output stream (tow_ms, sflags) per entry.
//
// Layout: one LANE per channel (as trk_lane.hip), not one wavefront per channel as the other telemetry kernels.  Reasons:
//   access   entries are [r · max_channels + c].  A wavefront that walks one channel reads 64 rounds at a stride of
//            max_channels entries, one 64-byte line per lane; with 1000 symbols per channel-second, twenty times LNAV's, that
//            traffic is the whole cost.  With a lane per channel the 64 lanes of a wave read 64 neighbouring entries of one
//            round: one line for floats.
//   serial   the stamp is a chain of double additions (+ 0.001 per symbol, not a multiple of anything) and a half-bit is a
//            chain of ten double additions in order: neither has a closed form, so a channel's symbols are consumed in order
//            anyway.  Everything between two decodes is a few integer operations per symbol.
//   state    per lane in registers: counters, the stamp, one double sum, two 170-bit half-bit strings ("sum > 0", "sum < 0":
//            the polarity, known only at the decode, picks one; both are cleared after it, so outside state 2 they are zero), and — in states 0 and 1 only — the 300 "< 0" bits of the
//            history's oldest entries as five 64-bit words that shift by one per symbol.  No array is indexed by a
//            run-time value: the kernel uses no scratch.
//   history  sign bits only, a ring of 2000 bits per channel in HBM (63 words).  The word being filled lives in a register
//            and is stored when it is complete or the run ends; it is loaded first, because its upper bits still hold the
//            oldest entries.  State 2 never looks at the correlation except on the decode symbol: it does not keep the
//            300-bit window, and the decode (or the first symbol after state 2 is left) gathers it from the ring.
//   hits     popcount of (window XOR time mark): 0 or 300 is a hit, below 150 is corr > 0.
// Every ring index is a counter reduced modulo 2000 and every record slot is below strings_per_run: no index comes from a
// symbol's value.
// The host path around the kernel (staging, the run calls' checks, output copies) is tlm_host.h, shared with the other
// four decoders; the device helpers of their kernels (tlm_device.h) have no use here.
#include <new>

#include "tlm_host.h"

using namespace gnsship;

namespace {

constexpr int kGnavRing = 2000;            // GLONASS_GNAV_STRING_SYMBOLS, GLONASS_GNAV_PREAMBLE_PERIOD_SYMBOLS
constexpr int kGnavPre = 300;              // GLONASS_GNAV_PREAMBLE_LENGTH_SYMBOLS
constexpr int kGnavData = 1700;            // GLONASS_GNAV_DATA_SYMBOLS
constexpr int kGnavCrcLimit = 6;           // CRC_ERROR_LIMIT
constexpr uint32_t kGnavMark = 0x3E375096u;  // "111110001101110101000010010110", the first bit in bit 29

// word w of the 300-bit string "the time mark wants a symbol < 0 here" (a 0 bit of the mark), symbol i in bit i
constexpr uint64_t gnav_mark_neg(int w)
{
    uint64_t v = 0;
    for (int b = 0; b < 64; b++) {
        const int i = 64 * w + b;
        if (i < kGnavPre && ((kGnavMark >> (29 - i / 10)) & 1u) == 0u) v |= 1ull << b;
    }
    return v;
}
constexpr uint64_t kMark0 = gnav_mark_neg(0), kMark1 = gnav_mark_neg(1), kMark2 = gnav_mark_neg(2), kMark3 = gnav_mark_neg(3), kMark4 = gnav_mark_neg(4);
constexpr uint64_t kWin4Mask = (1ull << 44) - 1ull;  // 300 − 256 bits

// The ICD's check relations as masks over the 85-bit word (bit i is bits[i]): beta_k and the information bits it covers.
__device__ __forceinline__ uint32_t gnav_parity(uint64_t lo, uint32_t hi, uint64_t mask_lo, uint32_t mask_hi)
{
    return static_cast<uint32_t>((__popcll(lo & mask_lo) + __popc(hi & mask_hi)) & 1);
}

struct GnavArgs {
    const float* sym;              // n_rounds × max_channels, or null
    const uint8_t* valid;          // the same shape, or null
    const gnsship_trk_epoch* rec;  // the same shape, or null (then sym)
    gnsship_gnav_state* chans;
    gnsship_gnav_string* strings;  // max_channels × strings_per_run
    int32_t* counts;
    uint32_t* tow_ms;              // max_rounds × max_channels
    uint8_t* sflags;               // the same shape
    int32_t max_channels, n_rounds, strings_per_run;
};

// 32 ring bits from position p (0..1999) on, wrapping at 2000; word `ci` of the ring is in `cur`, not yet in memory
__device__ __forceinline__ uint32_t gnav_ring32(const uint32_t* hist, int p, int ci, uint32_t cur)
{
    const int w = p >> 5, s = p & 31;
    const uint32_t a = w == ci ? cur : hist[w];
    const int w1 = w + 1 < 63 ? w + 1 : 0;  // only used where it is the word after w
    const uint32_t b = w1 == ci ? cur : hist[w1];
    uint32_t v = static_cast<uint32_t>(((static_cast<uint64_t>(b) << 32) | a) >> s);
    const int left = kGnavRing - p;  // bits before the wrap
    if (left < 32) {
        const uint32_t c = ci == 0 ? cur : hist[0];
        v = (v & ((1u << left) - 1u)) | (c << left);  // word 62 holds 16 bits: 1 <= left <= 31 here
    }
    return v;
}

// the field of `len` (<= 32) bits whose first (most significant) bit is bits[85 − first], as read_navigation_unsigned
__device__ __forceinline__ uint32_t gnav_field(uint64_t lo, uint32_t hi, int first, int len)
{
    const int s = 86 - first - len;  // the field's lowest bit, 0..84
    uint64_t v;
    if (s == 0) v = lo;
    else if (s < 64) v = (lo >> s) | (static_cast<uint64_t>(hi) << (64 - s));
    else v = static_cast<uint64_t>(hi) >> (s - 64);
    return static_cast<uint32_t>(v & ((1ull << len) - 1ull));
}

__device__ __forceinline__ uint32_t gnav_bit(uint64_t w0, uint64_t w1, uint64_t w2, int i)
{
    const uint64_t w = i < 64 ? w0 : (i < 128 ? w1 : w2);
    return static_cast<uint32_t>(w >> (i & 63)) & 1u;
}

// glot_to_gpst(t_k + 10, ...) before the fractional corrections: the week and the whole seconds of week
__device__ __forceinline__ void gnav_glot_to_gpst(uint32_t n_4, uint32_t n_t, uint32_t t_k, int32_t* wn, int64_t* tow)
{
    // days from 6 January 1980 to 1 January of 1996 + 4 (N_4 − 1) = 1992 + 4 N_4; 2100 is no leap year
    const int64_t year_day = 4378 + 1461 * static_cast<int64_t>(n_4) - (n_4 >= 28u ? 1 : 0);
    const int64_t utc = (year_day + static_cast<int64_t>(n_t) - 1) * 86400 + (static_cast<int64_t>(t_k) + 10 - 10800);  // > 0
    const int64_t d = utc / 86400;  // the UTC date
    const int64_t leap = d >= 13510 ? 18 : d >= 12960 ? 17 : d >= 11865 ? 16 : d >= 10588 ? 15 : d >= 9492 ? 14 : d >= 6935 ? 13 : d >= 6386 ? 12 :
        d >= 5839 ? 11 : d >= 5290 ? 10 : d >= 4925 ? 9 : d >= 4560 ? 8 : 7;  // the earliest instant, 30 December 1991, is after 1 January 1991
    const int64_t total = d * 86400 + (utc + leap) % 86400;  // days of the UTC date, seconds of day of the GPS instant
    *wn = static_cast<int32_t>(total / 604800);
    *tow = total % 604800;
}

__global__ __launch_bounds__(64) void gnav_kernel(const GnavArgs a)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= a.max_channels) return;
    gnsship_gnav_state* cs = a.chans + c;
    uint32_t* hist = cs->history;

    uint64_t counter = cs->symbol_counter, pi = cs->preamble_index;
    double tow_cur = cs->tow_at_current_symbol, tow = cs->tow, tau_c = cs->tau_c, tau_gps = cs->tau_gps, acc = cs->chip_acc;
    int stat = min(max(cs->stat, 0), 2), crc_err = cs->crc_error_counter, prn = cs->prn, wn = cs->wn;
    int size = static_cast<int>(counter < static_cast<uint64_t>(kGnavRing) ? counter : static_cast<uint64_t>(kGnavRing));
    uint32_t t_k = cs->t_k, t_b = cs->t_b, prev_tb = cs->previous_tb, n_t = cs->n_t, n_sat = cs->n, n_4 = cs->n_4;
    bool frame_sync = cs->frame_sync != 0, e1 = cs->ephemeris_str[0] != 0, e2 = cs->ephemeris_str[1] != 0, e3 = cs->ephemeris_str[2] != 0,
         e4 = cs->ephemeris_str[3] != 0, utc5 = cs->utc_model_str_5 != 0, tow_set = cs->tow_set != 0, tow_new = cs->tow_new != 0;
    uint64_t hp0 = cs->half_pos[0] | (static_cast<uint64_t>(cs->half_pos[1]) << 32), hp1 = cs->half_pos[2] | (static_cast<uint64_t>(cs->half_pos[3]) << 32),
             hp2 = cs->half_pos[4] | (static_cast<uint64_t>(cs->half_pos[5]) << 32);
    uint64_t hn0 = cs->half_neg[0] | (static_cast<uint64_t>(cs->half_neg[1]) << 32), hn1 = cs->half_neg[2] | (static_cast<uint64_t>(cs->half_neg[3]) << 32),
             hn2 = cs->half_neg[4] | (static_cast<uint64_t>(cs->half_neg[5]) << 32);

    int wp = static_cast<int>(counter % static_cast<uint64_t>(kGnavRing));  // the ring position of the newest entry
    int ci = wp >> 5;                                                       // the word in the register
    uint32_t cur = hist[ci];
    uint64_t w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0;  // the window: bit i is "< 0" of the i-th oldest entry
    bool win = false;                                  // ... when it is kept
    int in_idx = -1;                                   // the ring word the window's next bit comes from
    uint32_t in_word = 0;

    int count = 0;
    for (int r = 0; r < a.n_rounds; r++) {
        const size_t e = static_cast<size_t>(r) * a.max_channels + c;
        bool v = true;
        double x = 0.0;
        uint64_t sc = 0;
        if (a.rec) {
            v = (a.rec[e].flags & 1) != 0;
            if (v) {
                x = a.rec[e].prompt_i;
                sc = a.rec[e].sample_counter;
            }
        } else {
            if (a.valid) v = a.valid[e] != 0;
            if (v) x = static_cast<double>(a.sym[e]);
        }
        uint32_t out_tow = 0;
        uint8_t out_sf = 0;
        if (v) {
            // push
            counter++;
            const bool was_full = size == kGnavRing;
            if (!was_full) size++;
            wp = wp + 1 == kGnavRing ? 0 : wp + 1;
            if ((wp >> 5) != ci) {
                hist[ci] = cur;
                ci = wp >> 5;
                cur = hist[ci];
            }
            cur = (cur & ~(1u << (wp & 31))) | ((x < 0.0 ? 1u : 0u) << (wp & 31));

            // the correlation over the 300 oldest entries, where a state looks at it
            const bool due = stat == 2 && counter == pi + static_cast<uint64_t>(kGnavRing);
            int differ = 150;  // corr = 300 − 2 · differ; without 300 entries corr is 0
            if (size >= kGnavPre && (stat != 2 || due)) {
                int oldest = wp - size + 1;
                if (oldest < 0) oldest += kGnavRing;
                if (!win) {
                    uint32_t g[10];  // constant indices after unrolling
#pragma unroll
                    for (int k = 0; k < 10; k++) {
                        int p = oldest + 32 * k;
                        if (p >= kGnavRing) p -= kGnavRing;
                        g[k] = gnav_ring32(hist, p, ci, cur);
                    }
                    w0 = g[0] | (static_cast<uint64_t>(g[1]) << 32);
                    w1 = g[2] | (static_cast<uint64_t>(g[3]) << 32);
                    w2 = g[4] | (static_cast<uint64_t>(g[5]) << 32);
                    w3 = g[6] | (static_cast<uint64_t>(g[7]) << 32);
                    w4 = (g[8] | (static_cast<uint64_t>(g[9]) << 32)) & kWin4Mask;
                    win = true;
                    in_idx = -1;
                } else if (was_full) {  // the oldest entry left: the window moves on by one
                    int p = oldest + (kGnavPre - 1);
                    if (p >= kGnavRing) p -= kGnavRing;
                    if ((p >> 5) != in_idx) {
                        in_idx = p >> 5;
                        in_word = in_idx == ci ? cur : hist[in_idx];
                    }
                    const uint64_t nb = (in_word >> (p & 31)) & 1u;
                    w0 = (w0 >> 1) | (w1 << 63);
                    w1 = (w1 >> 1) | (w2 << 63);
                    w2 = (w2 >> 1) | (w3 << 63);
                    w3 = (w3 >> 1) | (w4 << 63);
                    w4 = (w4 >> 1) | (nb << 43);
                }
                differ = __popcll(w0 ^ kMark0) + __popcll(w1 ^ kMark1) + __popcll(w2 ^ kMark2) + __popcll(w3 ^ kMark3) + __popcll((w4 ^ kMark4) & kWin4Mask);
            }
            const bool hit = size >= kGnavPre && (differ == 0 || differ == kGnavPre);

            bool flag_preamble = false, decoded = false, inverted = false;
            if (stat == 0) {
                if (hit) {
                    pi = counter;
                    stat = 1;
                }
            } else if (stat == 1) {
                if (hit) {
                    const int32_t diff = static_cast<int32_t>(counter - pi);
                    if (diff == kGnavRing) {
                        pi = counter;
                        stat = 2;
                    } else if (diff > kGnavRing) {
                        stat = 0;
                    }
                }
            } else {
                // data symbol j of the string in flight
                const uint64_t j64 = counter - pi - static_cast<uint64_t>(kGnavPre + 1);
                if (j64 < static_cast<uint64_t>(kGnavData)) {
                    const uint32_t j = static_cast<uint32_t>(j64), h = j / 10u, k = j - 10u * h;
                    if (k == 0u) acc = 0.0;
                    acc = acc + x;
                    if (k == 9u) {
                        const uint64_t bit = 1ull << (h & 63u);
                        const uint64_t ps = acc > 0.0 ? bit : 0ull, ng = acc < 0.0 ? bit : 0ull;
                        if (h < 64u) {
                            hp0 = (hp0 & ~bit) | ps;
                            hn0 = (hn0 & ~bit) | ng;
                        } else if (h < 128u) {
                            hp1 = (hp1 & ~bit) | ps;
                            hn1 = (hn1 & ~bit) | ng;
                        } else {
                            hp2 = (hp2 & ~bit) | ps;
                            hn2 = (hn2 & ~bit) | ng;
                        }
                        acc = 0.0;
                    }
                }
                if (due) {
                    decoded = true;
                    inverted = !(differ < 150);  // corr_value > 0 is normal
                    const uint64_t h0 = inverted ? hn0 : hp0, h1 = inverted ? hn1 : hp1, h2 = inverted ? hn2 : hp2;
                    // half-bit pairs → relative bits → data bits; character i is bit 84 − i
                    uint64_t lo = 0;
                    uint32_t hi = 0;
                    uint32_t rel_prev = gnav_bit(h0, h1, h2, 0) & (gnav_bit(h0, h1, h2, 1) ^ 1u);
                    for (int i = 1; i < 85; i++) {
                        const uint32_t rel = gnav_bit(h0, h1, h2, 2 * i) & (gnav_bit(h0, h1, h2, 2 * i + 1) ^ 1u);
                        const uint32_t dbit = rel_prev ^ rel;
                        const int b = 84 - i;
                        if (b < 64) lo |= static_cast<uint64_t>(dbit) << b;
                        else hi |= dbit << (b - 64);
                        rel_prev = rel;
                    }
                    // CRC_test
                    const uint32_t syn = gnav_parity(lo, hi, 0x55555556aaad5b01ull, 0xaaaabu) | (gnav_parity(lo, hi, 0x9999999b33366d02ull, 0xccccdu) << 1) |
                        (gnav_parity(lo, hi, 0xe1e1e1e3c3c78e04ull, 0x10f0f1u) << 2) | (gnav_parity(lo, hi, 0xfe01fe03fc07f008ull, 0xff01u) << 3) |
                        (gnav_parity(lo, hi, 0xfffe0003fff80010ull, 0x1f0001u) << 4) | (gnav_parity(lo, hi, 0xfffffffc00000020ull, 0x1u) << 5) |
                        (gnav_parity(lo, hi, 0x40ull, 0x1ffffeu) << 6);
                    const uint32_t q_par = static_cast<uint32_t>((__popcll(lo >> 8) + __popc(hi)) & 1);  // bits 8..84
                    const uint32_t c_sigma = q_par ^ static_cast<uint32_t>(__popcll(lo & 0xFFull) & 1);
                    bool crc_ok = false;
                    int flipped = -1;
                    if (syn == 0u && c_sigma == 0u) {
                        crc_ok = true;
                    } else if (c_sigma == 1u && __popc(syn) == 1) {
                        crc_ok = true;
                    } else if (c_sigma == 1u && q_par == 1u) {
                        if (syn < 85u) {
                            // GLONASS_GNAV_ECC_LOCATOR: 0 for 0, k for 2^k, the other syndromes in order from 8 on
                            const int lg = 31 - __clz(static_cast<int>(syn | 1u));
                            flipped = syn == 0u ? 0 : ((syn & (syn - 1u)) == 0u ? lg : static_cast<int>(syn) + 6 - lg);
                            if (flipped < 64) lo ^= 1ull << flipped;
                            else hi ^= 1u << (flipped - 64);
                            crc_ok = true;
                        }
                    }
                    const uint32_t string_id = gnav_field(lo, hi, 2, 4);
                    bool slot = false, stamped_tow = false;
                    if (crc_ok) {  // string_decoder
                        if (string_id == 1u) {
                            t_k = gnav_field(lo, hi, 10, 5) * 3600u + gnav_field(lo, hi, 15, 6) * 60u + gnav_field(lo, hi, 21, 1) * 30u;
                            e1 = true;
                        } else if (string_id == 2u) {
                            if (e1) {
                                t_b = gnav_field(lo, hi, 10, 7) * 900u;
                                e2 = true;
                            }
                        } else if (string_id == 3u) {
                            if (e2) e3 = true;
                        } else if (string_id == 4u) {
                            if (e3) {
                                n_t = gnav_field(lo, hi, 60, 11);
                                n_sat = gnav_field(lo, hi, 71, 5);
                                slot = true;
                                e4 = true;
                            }
                        } else if (string_id == 5u) {
                            if (e4) {
                                const uint32_t tc = gnav_field(lo, hi, 17, 32), tg = gnav_field(lo, hi, 55, 22);
                                const double mc = static_cast<double>(tc & 0x7FFFFFFFu) * 4.656612873077392578125e-10;   // 2^-31
                                const double mg = static_cast<double>(tg & 0x1FFFFFu) * 9.31322574615478515625e-10;     // 2^-30
                                tau_c = (tc >> 31) ? -mc : mc;
                                tau_gps = (tg >> 21) ? -mg : mg;
                                n_4 = gnav_field(lo, hi, 50, 5);
                                utc5 = true;
                                if (e1) {
                                    int64_t whole;
                                    gnav_glot_to_gpst(n_4, n_t, t_k, &wn, &whole);
                                    tow = static_cast<double>(whole);
                                    tow = tow + (tau_c + tau_gps);
                                    tow_set = true;
                                    tow_new = true;
                                }
                            }
                        }
                    }
                    // have_new_ephemeris(), have_new_utc_model()
                    bool new_eph = false;
                    if (e1 && e2 && e3 && e4 && utc5 && prev_tb != t_b) {
                        e1 = e2 = e3 = e4 = false;
                        prev_tb = t_b;
                        new_eph = true;
                    }
                    const bool new_utc = utc5;
                    utc5 = false;
                    if (slot) prn = static_cast<int>(n_sat);
                    hp0 = hp1 = hp2 = hn0 = hn1 = hn2 = 0ull;  // the next string starts from nothing, in whatever state
                    acc = 0.0;
                    pi = counter;
                    if (crc_ok) {
                        crc_err = 0;
                        flag_preamble = true;
                        frame_sync = true;
                    } else {
                        crc_err++;
                        if (crc_err > kGnavCrcLimit) {
                            frame_sync = false;
                            stat = 0;
                        }
                    }
                    stamped_tow = flag_preamble && tow_new;
                    // the stamp of this symbol
                    if (stamped_tow) {
                        tow_cur = floor((tow - 0.3) * 1000.0) / 1000.0;
                        tow_new = false;
                    } else {
                        tow_cur = tow_cur + 0.001;
                    }
                    out_tow = static_cast<uint32_t>(static_cast<uint64_t>(static_cast<int64_t>(round(tow_cur * 1000.0))));
                    if (count < a.strings_per_run) {
                        gnsship_gnav_string* s = a.strings + (static_cast<size_t>(c) * a.strings_per_run + count);
                        s->symbol_counter = counter;
                        s->sample_counter = a.rec ? sc : 0ull;
                        s->tow = tow;
                        s->bits[0] = static_cast<uint32_t>(lo);
                        s->bits[1] = static_cast<uint32_t>(lo >> 32);
                        s->bits[2] = hi;
                        s->channel = c;
                        s->prn = prn;
                        s->string_id = static_cast<int32_t>(string_id);
                        s->flipped_bit = flipped;
                        s->tow_at_current_symbol_ms = out_tow;
                        s->flags = (crc_ok ? GNSSHIP_GNAV_CRC_OK : 0) | (flipped >= 0 ? GNSSHIP_GNAV_CORRECTED : 0) | (inverted ? GNSSHIP_GNAV_INVERTED : 0) |
                            (stamped_tow ? GNSSHIP_GNAV_NEW_TOW : 0) | (slot ? GNSSHIP_GNAV_SLOT_UPDATED : 0) | (new_eph ? GNSSHIP_GNAV_NEW_EPHEMERIS : 0) |
                            (new_utc ? GNSSHIP_GNAV_NEW_UTC_MODEL : 0);
                        s->reserved = 0;
                        count++;
                    }
                }
            }
            if (stat == 2) win = false;  // state 2 does not keep the window; the decode gathers it, and keeps it if it leaves state 2
            if (!decoded) {
                tow_cur = tow_cur + 0.001;
                out_tow = static_cast<uint32_t>(static_cast<uint64_t>(static_cast<int64_t>(round(tow_cur * 1000.0))));
            }
            out_sf = (frame_sync && tow_set ? GNSSHIP_GNAV_S_VALID_WORD : 0) | (decoded ? GNSSHIP_GNAV_S_STRING : 0) | (decoded && inverted ? GNSSHIP_GNAV_S_INVERTED : 0);
        }
        a.tow_ms[e] = out_tow;
        a.sflags[e] = out_sf;
    }

    hist[ci] = cur;
    cs->symbol_counter = counter;
    cs->preamble_index = pi;
    cs->tow_at_current_symbol = tow_cur;
    cs->tow = tow;
    cs->tau_c = tau_c;
    cs->tau_gps = tau_gps;
    cs->chip_acc = acc;
    cs->stat = stat;
    cs->crc_error_counter = crc_err;
    cs->history_size = size;
    cs->prn = prn;
    cs->wn = wn;
    cs->t_k = t_k;
    cs->t_b = t_b;
    cs->previous_tb = prev_tb;
    cs->n_t = n_t;
    cs->n = n_sat;
    cs->n_4 = n_4;
    cs->frame_sync = frame_sync;
    cs->ephemeris_str[0] = e1;
    cs->ephemeris_str[1] = e2;
    cs->ephemeris_str[2] = e3;
    cs->ephemeris_str[3] = e4;
    cs->utc_model_str_5 = utc5;
    cs->tow_set = tow_set;
    cs->tow_new = tow_new;
    cs->half_pos[0] = static_cast<uint32_t>(hp0);
    cs->half_pos[1] = static_cast<uint32_t>(hp0 >> 32);
    cs->half_pos[2] = static_cast<uint32_t>(hp1);
    cs->half_pos[3] = static_cast<uint32_t>(hp1 >> 32);
    cs->half_pos[4] = static_cast<uint32_t>(hp2);
    cs->half_pos[5] = static_cast<uint32_t>(hp2 >> 32);
    cs->half_neg[0] = static_cast<uint32_t>(hn0);
    cs->half_neg[1] = static_cast<uint32_t>(hn0 >> 32);
    cs->half_neg[2] = static_cast<uint32_t>(hn1);
    cs->half_neg[3] = static_cast<uint32_t>(hn1 >> 32);
    cs->half_neg[4] = static_cast<uint32_t>(hn2);
    cs->half_neg[5] = static_cast<uint32_t>(hn2 >> 32);
    a.counts[c] = count;
}

// what 1: set_satellite(prn); 2: a new object on prn.  One thread per channel of [first, first + n).
__global__ void gnav_control_kernel(gnsship_gnav_state* chans, int first, int n, int what, int prn)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    gnsship_gnav_state* cs = chans + first + i;
    if (what == 2) {
        gnsship_gnav_state z = {};
        *cs = z;
    }
    cs->prn = prn;
}

}  // namespace

struct gnsship_gnav {
    TlmHost h;  // h.mask: unused, the blocks never read Flag_valid_symbol_output
    gnsship_gnav_conf conf = {};
    int32_t strings_per_run = 0;
    gnsship_gnav_state* chans_dev = nullptr;
    gnsship_gnav_string* strings_dev = nullptr;
    int32_t* counts_dev = nullptr;
    uint32_t* tow_dev = nullptr;
    uint8_t* sflags_dev = nullptr;
};

extern "C" int gnsship_gnav_destroy(gnsship_gnav* t)
{
    if (!t) return GNSSHIP_E_INVAL;
    t->h.release_all({t->chans_dev, t->strings_dev, t->counts_dev, t->tow_dev, t->sflags_dev});
    delete t;
    return GNSSHIP_OK;
}

static int gnav_control(gnsship_gnav* t, int first, int n, int what, int prn, const char* who)
{
    hipLaunchKernelGGL(gnav_control_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, t->h.ctx->stream, t->chans_dev, first, n, what, prn);
    return launched(t->h.ctx, who);
}

extern "C" int gnsship_gnav_create(gnsship_ctx* ctx, const gnsship_gnav_conf* conf, int32_t max_channels, gnsship_gnav** out)
{
    if (!ctx || !out) return GNSSHIP_E_INVAL;
    *out = nullptr;
    if (!conf) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_gnav_create: null configuration");
    if (conf->max_rounds < 1 || conf->max_rounds > GNSSHIP_GNAV_MAX_ROUNDS) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_gnav_create: 1 <= max_rounds <= 2^20");
    if (conf->signal != GNSSHIP_GNAV_L1CA && conf->signal != GNSSHIP_GNAV_L2CA)
        return fail(ctx, GNSSHIP_E_INVAL, "gnsship_gnav_create: signal must be GNSSHIP_GNAV_L1CA or GNSSHIP_GNAV_L2CA");
    if (conf->reserved != 0) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_gnav_create: reserved must be 0");
    if (max_channels < 1 || max_channels > GNSSHIP_GNAV_MAX_CHANNELS) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_gnav_create: 1 <= max_channels <= 2^20");
    if (int rc = set_device(ctx)) return rc;
    gnsship_gnav* t = new (std::nothrow) gnsship_gnav();
    if (!t) return GNSSHIP_E_NOMEM;
    t->h.ctx = ctx;
    t->h.max_channels = max_channels;
    t->h.max_rounds = conf->max_rounds;
    t->conf = *conf;
    t->strings_per_run = GNSSHIP_GNAV_STRINGS_PER_RUN(conf->max_rounds);
    const size_t nc = static_cast<size_t>(max_channels), slots = nc * t->strings_per_run, entries = nc * conf->max_rounds;
    const hipError_t e = alloc_all(ctx, {dev_alloc(&t->chans_dev, nc, false), dev_alloc(&t->strings_dev, slots, true), dev_alloc(&t->counts_dev, nc, true),
                                            dev_alloc(&t->tow_dev, entries, true), dev_alloc(&t->sflags_dev, entries, true)});
    if (e != hipSuccess) {
        gnsship_gnav_destroy(t);
        return hip_fail(ctx, e, "gnsship_gnav_create");
    }
    if (int rc = gnav_control(t, 0, max_channels, 2, 0, "gnsship_gnav_create")) {  // every channel a new object on PRN 0
        gnsship_gnav_destroy(t);
        return rc;
    }
    *out = t;
    return GNSSHIP_OK;
}

// Launch over n_rounds entries per channel already on the device, then copy what the caller wants.
static int gnav_launch(gnsship_gnav* t, const float* sym, const uint8_t* valid, const gnsship_trk_epoch* rec, int32_t n_rounds,
    gnsship_gnav_string* strings_host, int32_t* counts_host, uint32_t* tow_ms_host, uint8_t* sflags_host, const char* who)
{
    gnsship_ctx* ctx = t->h.ctx;
    GnavArgs a = {};
    a.sym = sym;
    a.valid = valid;
    a.rec = rec;
    a.chans = t->chans_dev;
    a.strings = t->strings_dev;
    a.counts = t->counts_dev;
    a.tow_ms = t->tow_dev;
    a.sflags = t->sflags_dev;
    a.max_channels = t->h.max_channels;
    a.n_rounds = n_rounds;
    a.strings_per_run = t->strings_per_run;
    hipLaunchKernelGGL(gnav_kernel, dim3(static_cast<unsigned>((t->h.max_channels + 63) / 64)), dim3(64), 0, ctx->stream, a);  // a lane per channel
    if (int rc = launched(ctx, who)) return rc;
    const size_t nc = static_cast<size_t>(t->h.max_channels), slots = nc * t->strings_per_run, entries = nc * n_rounds;
    return copy_out(ctx, {{strings_host, t->strings_dev, sizeof(gnsship_gnav_string) * slots}, {counts_host, t->counts_dev, sizeof(int32_t) * nc},
                                 {tow_ms_host, t->tow_dev, sizeof(uint32_t) * entries}, {sflags_host, t->sflags_dev, entries}}, who);
}

extern "C" int gnsship_gnav_run_symbols(gnsship_gnav* t, const float* symbols, const uint8_t* valid, const uint8_t* out_valid, int on_device,
    int32_t n_rounds, gnsship_gnav_string* strings_host, int32_t* counts_host, uint32_t* tow_ms_host, uint8_t* sflags_host)
{
    if (!t) return GNSSHIP_E_INVAL;
    (void)out_valid;  // Flag_valid_symbol_output: the blocks never read it
    const char* who = "gnsship_gnav_run_symbols";
    if (int rc = tlm_symbols_in(t->h, who, on_device, n_rounds, &symbols, &valid, nullptr)) return rc;
    return gnav_launch(t, symbols, valid, nullptr, n_rounds, strings_host, counts_host, tow_ms_host, sflags_host, who);
}

extern "C" int gnsship_gnav_run_records(gnsship_gnav* t, const gnsship_trk_epoch* records, int on_device, int32_t n_rounds,
    gnsship_gnav_string* strings_host, int32_t* counts_host, uint32_t* tow_ms_host, uint8_t* sflags_host)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_gnav_run_records";
    if (int rc = tlm_records_in(t->h, who, on_device, n_rounds, &records)) return rc;
    return gnav_launch(t, nullptr, nullptr, records, n_rounds, strings_host, counts_host, tow_ms_host, sflags_host, who);
}

extern "C" int gnsship_gnav_run_trk(gnsship_gnav* t, gnsship_trk* trk, gnsship_gnav_string* strings_host, int32_t* counts_host,
    uint32_t* tow_ms_host, uint8_t* sflags_host, int32_t* n_rounds_out)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_gnav_run_trk";
    const gnsship_trk_epoch* rec = nullptr;
    int32_t rounds = 0;
    if (int rc = tlm_trk_in(t->h, who, trk, &rec, &rounds)) return rc;
    if (n_rounds_out) *n_rounds_out = rounds;
    return gnav_launch(t, nullptr, nullptr, rec, rounds, strings_host, counts_host, tow_ms_host, sflags_host, who);
}

extern "C" int gnsship_gnav_outputs_device(gnsship_gnav* t, gnsship_gnav_string** strings, int32_t** counts, uint32_t** tow_ms, uint8_t** sflags,
    int32_t* strings_per_run)
{
    if (!t) return GNSSHIP_E_INVAL;
    if (strings) *strings = t->strings_dev;
    if (counts) *counts = t->counts_dev;
    if (tow_ms) *tow_ms = t->tow_dev;
    if (sflags) *sflags = t->sflags_dev;
    if (strings_per_run) *strings_per_run = t->strings_per_run;
    return GNSSHIP_OK;
}

// set_satellite (what 1) and new_channel (2) on one channel
static int gnav_channel_call(gnsship_gnav* t, int32_t channel, int what, int32_t prn, const char* who)
{
    if (!t) return GNSSHIP_E_INVAL;
    if (int rc = tlm_check_channel(t->h, who, channel)) return rc;
    if (prn < 0 || prn > 63) return reject(t->h.ctx, GNSSHIP_E_INVAL, who, "0 <= prn <= 63");
    if (int rc = set_device(t->h.ctx)) return rc;
    return gnav_control(t, channel, 1, what, prn, who);
}

extern "C" int gnsship_gnav_set_satellite(gnsship_gnav* t, int32_t channel, int32_t prn)
{
    return gnav_channel_call(t, channel, 1, prn, "gnsship_gnav_set_satellite");
}

extern "C" int gnsship_gnav_new_channel(gnsship_gnav* t, int32_t channel, int32_t prn)
{
    return gnav_channel_call(t, channel, 2, prn, "gnsship_gnav_new_channel");
}

extern "C" int gnsship_gnav_state_get(gnsship_gnav* t, int32_t channel, gnsship_gnav_state* st)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_gnav_state_get";
    if (int rc = tlm_check_state(t->h, who, channel, st)) return rc;
    if (int rc = set_device(t->h.ctx)) return rc;
    return copy_out(t->h.ctx, {{st, &t->chans_dev[channel], sizeof(*st)}}, who);
}

extern "C" int gnsship_gnav_state_set(gnsship_gnav* t, int32_t channel, const gnsship_gnav_state* st)
{
    if (!t) return GNSSHIP_E_INVAL;
    gnsship_ctx* ctx = t->h.ctx;
    if (int rc = tlm_check_state(t->h, "gnsship_gnav_state_set", channel, st)) return rc;
    const uint64_t full = st->symbol_counter < 2000u ? st->symbol_counter : 2000u;
    const uint8_t flags[] = {st->frame_sync, st->ephemeris_str[0], st->ephemeris_str[1], st->ephemeris_str[2], st->ephemeris_str[3], st->utc_model_str_5,
        st->tow_set, st->tow_new};
    bool ok = st->stat >= 0 && st->stat <= 2 && st->history_size >= 0 && static_cast<uint64_t>(st->history_size) == full && st->crc_error_counter >= 0;
    for (uint8_t f : flags) ok = ok && f <= 1;
    if (!ok) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_gnav_state_set: stat 0..2, history_size == min(symbol_counter, 2000), crc_error_counter >= 0, flags 0 or 1");
    if (int rc = set_device(ctx)) return rc;
    // pageable host memory: the copy has left *st when the call returns, and is ordered on the stream
    const hipError_t e = hipMemcpyAsync(&t->chans_dev[channel], st, sizeof(*st), hipMemcpyHostToDevice, ctx->stream);
    return e == hipSuccess ? GNSSHIP_OK : hip_fail(ctx, e, "gnsship_gnav_state_set");
}
