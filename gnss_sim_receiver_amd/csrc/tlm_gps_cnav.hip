// tlm_gps_cnav.hip — gps_l2c_telemetry_decoder_gs and gps_l5_telemetry_decoder_gs on the device up to the time of week
// (include/gnsship.h, gnsship_cnav_*): libswiftcnav's two streaming K=7 Viterbi decoders one symbol apart, the preamble
// rescan, CRC-24Q, the lock counter, the precedence of part 1, and each block's watchdog, TOW stamp and valid_word.  One
// kernel serves both signals; `signal` selects the block-level differences.  Input: floats with a validity and an
// output-valid mask, or tracking's epoch records (host, device, or in place where gnsship_trk left them).  Output: one
// record per 300-bit buffer a locked part disposed of, the block's output stream (tow_ms, sflags) per entry, and
// per-channel fault flags.
//
// Layout: one workgroup of one wavefront per channel, as tlm_gps_lnav.hip and for its reason: a channel's symbols are
// strictly ordered and each part's next step depends on the last verdict.
//   trellis   the 64 lanes are the 64 states: lane j holds old_metrics[j] and new_metrics[j] (the stale buffer the
//             chain-back reads) of both parts in registers.  One add-compare-select step reads old[j >> 1] and
//             old[(j >> 1) + 32] across lanes, forms the two candidates as the reference's BFLY does (uint32, the decision
//             (int32)(m0 - m1) > 0), and one ballot of the decisions is the step's v27_decision_t: bit j is state j's.
//   ring      lane L keeps decisions[L] of each part in two registers; the step writes the ballot into the lane the
//             decision index names, the chain-back reads 64 of them back by wave-uniform lane reads.
//   buffers   in LDS for the run: each part's 128 symbols, and its 512-bit decode buffer as one byte per bit, so that the
//             append, the rescan (one candidate offset per lane, a ballot, find-first-set), the shift and the packing of
//             a message are lane-parallel.  CRC-24Q runs over five ballots of the bits in scalar registers.
//   gather    64 entries at a time; a ballot of the valid entries and a prefix popcount give each symbol its ordinal, and
//             lane k then stands for the chunk's k-th symbol.
//   machine   wave-uniform, from event to event: an event is a symbol at which a part's symbol buffer fills (or a locked
//             part holds 300 bits).  Between two events nothing moves but the symbol buffers, the counters and the TOW, so
//             every lane works out the tow_ms / sflags of its own symbol: for L5 in closed form, for L2C by the block's
//             own additions — one `+= 0.02` per symbol, in order, each lane keeping the sum that is its own.
//   both parts run in the same wave, one after the other; they share every symbol and either may flush the other.
// Every LDS and HBM index comes from lane numbers, counters and ballot bits, never from a symbol's value.
// The host path around the kernel (staging, the run calls' checks, output copies) is tlm_host.h.
#include <new>

#include "tlm_device.h"
#include "tlm_host.h"

using namespace gnsship;

namespace {

constexpr int kCnavMsgBits = 300;               // GPS_CNAV_MSG_LENGTH
constexpr int kCnavDataBits = 276;              // without the CRC
constexpr int kCnavBufBits = 512;               // the decode buffer, 64 bytes
constexpr int kCnavMaxHeld = 480;               // most bits a part may hold ahead of an append of 32
constexpr int kCnavMaxCrcFails = 10;            // GPS_CNAV_LOCK_MAX_CRC_FAILS
constexpr uint32_t kCnavPre1 = 0x8Bu, kCnavPre2 = 0x74u;
constexpr uint32_t kCnavNormLimit = 1u << 30;
constexpr uint64_t kCnavWatchdogL2c = 300 * 2 * 5, kCnavWatchdogL5 = 300 * 2 * 10;

struct CnavArgs {
    const float* sym;              // n_rounds × max_channels, or null
    const uint8_t* valid;          // the same shape, or null
    const uint8_t* out_valid;      // the same shape, or null
    const gnsship_trk_epoch* rec;  // the same shape, or null (then sym)
    gnsship_cnav_state* chans;
    gnsship_cnav_message* messages;  // max_channels × messages_per_run
    int32_t* counts;
    uint8_t* faults;
    uint32_t* tow_ms;              // max_rounds × max_channels
    uint8_t* sflags;               // the same shape
    int32_t max_channels, n_rounds, messages_per_run, signal;
};

struct CnavPart {  // one cnav_v27_part_t: four registers per lane, the rest wave-uniform
    uint32_t old, stale, dlo, dhi;
    int n_symbols, n_decoded, n_crc_fail, didx;
    bool old2, seen, invert, lock, crc_ok, init;
};

__device__ __forceinline__ uint32_t cnav_shfl(uint32_t v, int src) { return static_cast<uint32_t>(__shfl(static_cast<int>(v), src)); }
__device__ __forceinline__ uint32_t cnav_lane(uint32_t v, int src)  // src is wave-uniform
{
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), tlm_uniform(src)));
}
__device__ __forceinline__ uint32_t cnav_wave_min(uint32_t v)
{
    for (int off = 32; off > 0; off >>= 1) v = min(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), off)));
    return v;
}
__device__ __forceinline__ unsigned long long cnav_below(int x) { return x >= 64 ? ~0ull : (1ull << x) - 1ull; }  // bits [0, x)

__device__ __forceinline__ void cnav_load(CnavPart& p, const gnsship_cnav_part* s, uint8_t* sym, uint8_t* bit, int lane)
{
    p.old2 = tlm_uniform(static_cast<int>(s->old_is_metrics2)) != 0;
    p.old = s->metrics[p.old2 ? 1 : 0][lane];
    p.stale = s->metrics[p.old2 ? 0 : 1][lane];
    p.dlo = s->decisions[lane][0];
    p.dhi = s->decisions[lane][1];
    p.init = tlm_uniform(static_cast<int>(s->init)) != 0;
    p.n_symbols = static_cast<int>(min(tlm_uniform(s->n_symbols), p.init ? 127u : 63u));
    p.n_decoded = static_cast<int>(min(tlm_uniform(s->n_decoded), static_cast<uint32_t>(kCnavMaxHeld)));
    p.n_crc_fail = static_cast<int>(tlm_uniform(s->n_crc_fail));
    p.didx = static_cast<int>(tlm_uniform(s->decisions_index) & 63u);
    p.seen = tlm_uniform(static_cast<int>(s->preamble_seen)) != 0;
    p.invert = tlm_uniform(static_cast<int>(s->invert)) != 0;
    p.lock = tlm_uniform(static_cast<int>(s->message_lock)) != 0;
    p.crc_ok = tlm_uniform(static_cast<int>(s->crc_ok)) != 0;
    sym[lane] = s->symbols[lane];
    sym[lane + 64] = s->symbols[lane + 64];
    const uint32_t byte = s->decoded[lane];  // bits 8·lane .. 8·lane + 7, MSB first
    for (int t = 0; t < 8; t++) bit[8 * lane + t] = static_cast<uint8_t>((byte >> (7 - t)) & 1u);
}

__device__ __forceinline__ void cnav_store(const CnavPart& p, gnsship_cnav_part* s, const uint8_t* sym, const uint8_t* bit, int lane)
{
    s->metrics[p.old2 ? 1 : 0][lane] = p.old;
    s->metrics[p.old2 ? 0 : 1][lane] = p.stale;
    s->decisions[lane][0] = p.dlo;
    s->decisions[lane][1] = p.dhi;
    s->symbols[lane] = sym[lane];
    s->symbols[lane + 64] = sym[lane + 64];
    uint32_t byte = 0;
    for (int t = 0; t < 8; t++) byte |= static_cast<uint32_t>(bit[8 * lane + t] & 1u) << (7 - t);
    s->decoded[lane] = static_cast<uint8_t>(byte);
    if (lane == 0) {
        s->n_symbols = static_cast<uint32_t>(p.n_symbols);
        s->n_decoded = static_cast<uint32_t>(p.n_decoded);
        s->n_crc_fail = static_cast<uint32_t>(p.n_crc_fail);
        s->decisions_index = static_cast<uint32_t>(p.didx);
        s->old_is_metrics2 = p.old2;
        s->preamble_seen = p.seen;
        s->invert = p.invert;
        s->message_lock = p.lock;
        s->crc_ok = p.crc_ok;
        s->init = p.init;
        s->reserved[0] = s->reserved[1] = 0;
    }
}

// bitshl over the whole buffer: bit[i] = bit[i + shift], zero fill; 1 <= shift <= 512
__device__ __forceinline__ void cnav_shl(uint8_t* bit, int shift, int lane)
{
    uint8_t keep[8];
    for (int r = 0; r < 8; r++) {
        const int i = lane + 64 * r + shift;
        keep[r] = i < kCnavBufBits ? bit[i] : 0;
    }
    __syncthreads();
    for (int r = 0; r < 8; r++) bit[lane + 64 * r] = keep[r];
    __syncthreads();
}

// cnav_rescan_preamble_ (cnav_msg.c:117-145)
__device__ __forceinline__ void cnav_rescan(CnavPart& p, uint8_t* bit, int lane)
{
    p.seen = false;
    if (p.n_decoded > 9) {
        const int j = p.n_decoded - 8;  // candidates 1 <= i < j; i + 7 < n_decoded <= 512
        int found = 0;
        bool inv = false;
        for (int base = 1; base < j && found == 0; base += 64) {
            const int i = base + lane;
            uint32_t c = 0;
            if (i < j)
                for (int t = 0; t < 8; t++) c = (c << 1) | bit[i + t];
            const bool hit = i < j && (c == kCnavPre1 || c == kCnavPre2);
            const unsigned long long hits = __ballot(hit), inverted = __ballot(hit && c == kCnavPre2);
            if (hits) {
                const int l = __ffsll(hits) - 1;
                found = base + l;
                inv = ((inverted >> l) & 1ull) != 0;
            }
        }
        if (found > 0) {
            p.seen = true;
            p.invert = inv;
            cnav_shl(bit, found, lane);
            p.n_decoded -= found;
        }
    }
    if (!p.seen && p.n_decoded >= 8) {
        cnav_shl(bit, p.n_decoded - 7, lane);
        p.n_decoded = 7;
    }
}

// CRC-24Q over the first 276 bits against the last 24 (cnav_compute_crc_ / cnav_extract_crc_), both under `invert`
__device__ __forceinline__ bool cnav_crc_matches(const CnavPart& p, const uint8_t* bit, int lane)
{
    uint32_t crc = 0, sent = 0;
    for (int r = 0; r < 5; r++) {
        const unsigned long long w = __ballot(((bit[lane + 64 * r] & 1u) != 0) != p.invert);
        for (int t = 0; t < 64; t++) {
            const int i = 64 * r + t;
            const uint32_t b = static_cast<uint32_t>((w >> t) & 1ull);
            if (i < kCnavDataBits) {
                crc ^= b << 23;
                crc <<= 1;
                if (crc & 0x1000000u) crc ^= 0x1864CFBu;
            } else if (i < kCnavMsgBits) {
                sent = (sent << 1) | b;
            }
        }
    }
    return (crc & 0xFFFFFFu) == sent;
}

// v27_update over the held symbols, v27_chainback_likely over 64 bits, the oldest 32 appended, then the retry loop of
// cnav_add_symbol_ (cnav_msg.c:183-280).  Called when the symbol buffer is full.
__device__ __forceinline__ void cnav_decode(CnavPart& p, const uint8_t* sym, uint8_t* bit, int lane)
{
    const int nbits = p.n_symbols >> 1;
    const int i = lane >> 1;
    const uint32_t c0 = (__popc((2u * i) & 0x4Fu) & 1) ? 255u : 0u, c1 = (__popc((2u * i) & 0x6Du) & 1) ? 255u : 0u;  // v27_poly_init
    for (int b = 0; b < nbits; b++) {
        const uint32_t s0 = sym[2 * b], s1 = sym[2 * b + 1];
        const uint32_t metric = (c0 ^ s0) + (c1 ^ s1);
        uint32_t m0 = cnav_shfl(p.old, i) + metric, m1 = cnav_shfl(p.old, i + 32) + (510u - metric);
        if (lane & 1) {
            const uint32_t t = metric + metric - 510u;
            m0 -= t;
            m1 += t;
        }
        const bool decision = static_cast<int32_t>(m0 - m1) > 0;
        uint32_t nw = decision ? m1 : m0;
        const unsigned long long w = __ballot(decision);
        if (cnav_lane(nw, 0) > kCnavNormLimit) nw -= min(cnav_wave_min(nw), 1u << 31);  // state 0 alone is tested
        if (lane == p.didx) {
            p.dlo = static_cast<uint32_t>(w);
            p.dhi = static_cast<uint32_t>(w >> 32);
        }
        p.didx = (p.didx + 1) & 63;
        p.stale = p.old;  // the swap: new_metrics names the buffer this step read from
        p.old = nw;
        p.old2 = !p.old2;
    }
    p.n_symbols = 0;

    // the first minimum of the stale buffer starts the walk
    const uint32_t best = cnav_wave_min(p.stale);
    uint32_t s = static_cast<uint32_t>(__ffsll(__ballot(p.stale == best)) - 1);
    uint32_t word = 0;  // tmp_bits 0..31, MSB first
    int idx = p.didx;
    for (int nb = 63; nb >= 0; nb--) {
        idx = (idx + 63) & 63;
        const uint32_t d = cnav_lane((s & 32u) ? p.dhi : p.dlo, idx);
        const uint32_t k = (d >> (s & 31u)) & 1u;
        s = (s >> 1) | (k << 5);
        if (nb < 32) word |= k << (31 - nb);
    }
    if (lane < 32 && p.n_decoded + lane < kCnavBufBits) bit[p.n_decoded + lane] = static_cast<uint8_t>((word >> (31 - lane)) & 1u);
    p.n_decoded = min(p.n_decoded + 32, kCnavBufBits);  // n_decoded <= 480 before: the bound never binds
    __syncthreads();

    bool retry = true;
    while (retry) {
        retry = false;
        if (!p.seen) cnav_rescan(p, bit, lane);
        if (p.seen && p.n_decoded >= kCnavMsgBits) {
            const bool match = cnav_crc_matches(p, bit, lane);
            if (p.lock) {
                p.crc_ok = match;
                if (match) {
                    p.n_crc_fail = 0;
                } else if (++p.n_crc_fail > kCnavMaxCrcFails) {
                    p.n_crc_fail = 0;
                    p.lock = false;
                    p.seen = false;
                    retry = true;
                }
            } else if (match) {
                p.lock = true;
                p.crc_ok = true;
                p.n_crc_fail = 0;
            } else {
                p.crc_ok = false;
                p.seen = false;
                retry = true;
            }
        }
    }
}

// cnav_add_symbol_ for one symbol
__device__ __forceinline__ void cnav_add(CnavPart& p, uint8_t* sym, uint8_t* bit, uint8_t s, int lane)
{
    if (lane == 0) sym[p.n_symbols] = s;  // n_symbols <= 127
    p.n_symbols++;
    if (p.n_symbols < (p.init ? 128 : 64)) return;
    p.init = false;
    __syncthreads();
    cnav_decode(p, sym, bit, lane);
}

// The symbols [pos, ev) of the chunk, none of them an event, into one part's symbol buffer.  A flushed part (the other is
// locked) is zeroed after every symbol: each symbol lands at index 0 but the first, which lands at n_symbols.
__device__ __forceinline__ void cnav_plain(CnavPart& p, uint8_t* sym, bool flushed, uint8_t mine, int pos, int ev, int lane)
{
    if (!flushed) {
        if (lane >= pos && lane < ev) sym[p.n_symbols + (lane - pos)] = mine;  // < the threshold: no event before ev
        p.n_symbols += ev - pos;
        return;
    }
    if (lane == pos && (p.n_symbols != 0 || ev - pos == 1)) sym[p.n_symbols] = mine;
    if (lane == ev - 1 && ev - pos >= 2) sym[0] = mine;
    p.n_symbols = 0;
    p.n_decoded = 0;
}

__global__ __launch_bounds__(64) void cnav_kernel(const CnavArgs a)
{
    __shared__ uint8_t s_sym[2][128];
    __shared__ uint8_t s_bit[2][kCnavBufBits];
    __shared__ uint8_t c_sym[64], c_ov[64], o_sf[64];
    __shared__ uint32_t o_tow[64];
    __shared__ uint64_t c_sc[64];
    const int lane = threadIdx.x;
    const int c = blockIdx.x;  // the grid is max_channels workgroups
    const bool l5 = a.signal == GNSSHIP_CNAV_L5;
    const uint64_t limit = l5 ? kCnavWatchdogL5 : kCnavWatchdogL2c;

    gnsship_cnav_state* cs = a.chans + c;
    CnavPart p1, p2;
    cnav_load(p1, &cs->part[0], s_sym[0], s_bit[0], lane);
    cnav_load(p2, &cs->part[1], s_sym[1], s_bit[1], lane);
    uint64_t counter = tlm_uniform64(cs->symbol_counter), last_valid = tlm_uniform64(cs->last_valid_preamble);
    double tow_s = __longlong_as_double(static_cast<long long>(tlm_uniform64(static_cast<uint64_t>(__double_as_longlong(cs->tow_s)))));
    uint32_t tow_ms = tlm_uniform(cs->tow_ms), tow_pre = tlm_uniform(cs->tow_at_preamble);
    bool pll180 = tlm_uniform(static_cast<int>(cs->pll_180)) != 0, vw = tlm_uniform(static_cast<int>(cs->valid_word)) != 0;
    bool sent = tlm_uniform(static_cast<int>(cs->sent_tlm_failed)) != 0;
    __syncthreads();

    int count = 0;
    bool fault = false;
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
                    const double s = l5 ? a.rec[e].prompt_q : a.rec[e].prompt_i;  // asked of the double itself
                    code = s > 0.0 ? 255 : 0;
                    sc = a.rec[e].sample_counter;
                }
            } else {
                if (a.valid) v = a.valid[e] != 0;
                if (v) {
                    code = a.sym[e] > 0.0f ? 255 : 0;
                    if (a.out_valid) ov = a.out_valid[e] != 0;
                }
            }
        }
        const unsigned long long mask = __ballot(v);
        const int n = __popcll(mask);  // 0..64, wave-uniform
        const int ord = __popcll(mask & ((1ull << lane) - 1ull));
        if (n > 0) {
            if (v) {
                c_sym[ord] = code;
                c_ov[ord] = ov ? 1 : 0;
                c_sc[ord] = sc;
            }
            __syncthreads();
            // from here lane k stands for the chunk's k-th symbol
            const bool mine_is = lane < n;
            const uint8_t mine = mine_is ? c_sym[lane] : 0;
            const unsigned long long bad = __ballot(mine_is && c_ov[lane] == 0);
            uint32_t out_tow = 0;
            uint8_t out_sf = 0;

            int pos = 0;  // symbols [0, pos) of the chunk are done
            while (pos < n) {
                // the next event: a symbol buffer fills, or a locked part already holds a message
                const int flushed = p1.lock ? 1 : (p2.lock ? 0 : -1);
                int ev = n;
                if (flushed == 0) {
                    if (p1.n_symbols + 1 >= (p1.init ? 128 : 64)) ev = pos;
                } else {
                    ev = min(ev, pos + (p1.init ? 128 : 64) - p1.n_symbols - 1);
                }
                if (flushed == 1) {
                    if (p2.n_symbols + 1 >= (p2.init ? 128 : 64)) ev = pos;
                } else {
                    ev = min(ev, pos + (p2.init ? 128 : 64) - p2.n_symbols - 1);
                }
                if ((flushed == 1 && p1.n_decoded >= kCnavMsgBits) || (flushed == 0 && p2.n_decoded >= kCnavMsgBits)) ev = pos;

                if (ev > pos) {  // plain symbols pos .. ev − 1
                    cnav_plain(p1, s_sym[0], flushed == 0, mine, pos, ev, lane);
                    cnav_plain(p2, s_sym[1], flushed == 1, mine, pos, ev, lane);
                    counter += static_cast<uint64_t>(ev - pos);
                    if (!sent && counter - last_valid > limit) {
                        sent = true;
                        fault = true;
                    }
                    const bool in_range = lane >= pos && lane < ev;
                    const unsigned long long span = cnav_below(ev) & ~cnav_below(pos), rb = bad & span;
                    const bool ok_here = (rb & cnav_below(lane + 1)) == 0ull;  // no output-invalid entry up to this one
                    if (!l5) {
                        double mine_tow = 0.0;
                        for (int k = pos; k < ev; k++) {  // the block's own additions, in order
                            tow_s += 0.02;
                            if (lane == k) mine_tow = tow_s;
                        }
                        if (in_range) {
                            out_tow = static_cast<uint32_t>(round(mine_tow * 1000.0));
                            out_sf = ((vw && ok_here) ? 1 : 0) | (pll180 ? 2 : 0);
                        }
                    } else if (vw) {
                        const int first_bad = rb ? __ffsll(rb) - 1 : ev - 1;  // the last symbol that still adds its 10 ms
                        if (in_range && ok_here) {
                            out_tow = tow_ms + 10u * static_cast<uint32_t>(lane - pos + 1);
                            out_sf = 1 | (pll180 ? 2 : 0);
                        }
                        tow_ms += 10u * static_cast<uint32_t>(first_bad - pos + 1);
                    }
                    if (rb) vw = false;
                    pos = ev;
                    __syncthreads();
                }
                if (pos >= n) break;

                // ---- symbol `pos`: cnav_msg_decoder_add_symbol in full ----
                const uint8_t s = static_cast<uint8_t>(tlm_uniform(static_cast<int>(c_sym[pos])));
                const bool ov_here = ((bad >> pos) & 1ull) == 0ull;
                cnav_add(p1, s_sym[0], s_bit[0], s, lane);
                cnav_add(p2, s_sym[1], s_bit[1], s, lane);
                bool res = false;
                uint32_t msg_tow = 0, delay = 0;
                if (p1.lock || p2.lock) {
                    const int which = p1.lock ? 0 : 1;
                    CnavPart& p = which ? p2 : p1;
                    CnavPart& other = which ? p1 : p2;
                    uint8_t* bit = s_bit[which];
                    other.n_decoded = 0;
                    other.n_symbols = 0;
                    if (p.n_decoded >= kCnavMsgBits) {  // cnav_msg_decode_
                        __syncthreads();
                        const unsigned long long w0 = __ballot(((bit[lane] & 1u) != 0) != p.invert);  // bits 0..63, un-inverted
                        uint32_t prn = 0, msg_id = 0;
                        for (int t = 0; t < 6; t++) {
                            prn = (prn << 1) | static_cast<uint32_t>((w0 >> (8 + t)) & 1ull);
                            msg_id = (msg_id << 1) | static_cast<uint32_t>((w0 >> (14 + t)) & 1ull);
                        }
                        for (int t = 0; t < 17; t++) msg_tow = (msg_tow << 1) | static_cast<uint32_t>((w0 >> (20 + t)) & 1ull);
                        const uint32_t alert = static_cast<uint32_t>((w0 >> 37) & 1ull);
                        delay = static_cast<uint32_t>((p.n_decoded - kCnavMsgBits + 32) * 2 + p.n_symbols);
                        res = p.crc_ok;
                        if (count < a.messages_per_run) {
                            gnsship_cnav_message* m = a.messages + (static_cast<size_t>(c) * a.messages_per_run + count);
                            if (lane < 38) {
                                uint32_t byte = 0;
                                for (int t = 0; t < 8; t++) byte |= static_cast<uint32_t>(bit[8 * lane + t] & 1u) << (7 - t);
                                m->raw[lane] = static_cast<uint8_t>(p.invert ? byte ^ 0xFFu : byte);
                            }
                            if (lane == 0) {
                                m->symbol_counter = counter + 1u;
                                m->sample_counter = a.rec ? c_sc[pos] : 0ull;
                                m->channel = c;
                                m->tow = msg_tow;
                                m->delay = delay;
                                m->prn = static_cast<uint8_t>(prn);
                                m->msg_id = static_cast<uint8_t>(msg_id);
                                m->alert = static_cast<uint8_t>(alert);
                                m->part = static_cast<uint8_t>(which);
                                m->flags = static_cast<uint8_t>((p.crc_ok ? 1 : 0) | (p.invert ? 2 : 0) | (p.lock ? 4 : 0));
                                m->reserved = 0;
                            }
                            count++;
                        }
                        cnav_shl(bit, kCnavMsgBits, lane);
                        p.n_decoded -= kCnavMsgBits;
                    }
                }
                counter += 1u;
                if (!sent && counter - last_valid > limit) {
                    sent = true;
                    fault = true;
                }
                if (res) {
                    pll180 = p1.invert || p2.invert;  // the stale `invert` of the part that is not locked included
                    if (!l5) {
                        tow_pre = msg_tow;
                        last_valid = counter;
                        tow_s = static_cast<double>(msg_tow) * 6.0 + static_cast<double>(delay) * 0.02 + 12 * 0.02;
                        vw = true;
                    } else {
                        tow_pre = msg_tow * 6000u;
                        const uint32_t last = tow_ms;
                        tow_ms = msg_tow * 6000u + (delay + 12u) * 10u;
                        const int64_t diff = static_cast<int64_t>(tow_ms) - static_cast<int64_t>(last);
                        if (last != 0u && (diff < 0 ? -diff : diff) > 10) {
                            tow_ms = 0;
                            vw = false;
                        } else {
                            last_valid = counter;
                            vw = true;
                        }
                    }
                } else if (!l5) {
                    tow_s += 0.02;
                    if (!ov_here) vw = false;
                } else if (vw) {
                    tow_ms += 10u;
                    if (!ov_here) vw = false;
                }
                if (lane == pos) {
                    if (!l5) {
                        out_tow = static_cast<uint32_t>(round(tow_s * 1000.0));
                        out_sf = (vw ? 1 : 0) | (pll180 ? 2 : 0);
                    } else if (vw) {
                        out_tow = tow_ms;
                        out_sf = 1 | (pll180 ? 2 : 0);
                    }
                    if (res) out_sf |= 4;
                }
                pos++;
                __syncthreads();
            }
            // back to the entries: lane k's results belong to the entry whose ordinal is k
            o_tow[lane] = out_tow;
            o_sf[lane] = out_sf;
            __syncthreads();
        }
        if (in_run) {
            a.tow_ms[e] = (n > 0 && v) ? o_tow[ord] : 0u;
            a.sflags[e] = (n > 0 && v) ? o_sf[ord] : 0;
        }
        __syncthreads();
    }

    cnav_store(p1, &cs->part[0], s_sym[0], s_bit[0], lane);
    cnav_store(p2, &cs->part[1], s_sym[1], s_bit[1], lane);
    if (lane == 0) {
        cs->symbol_counter = counter;
        cs->last_valid_preamble = last_valid;
        cs->tow_s = tow_s;
        cs->tow_ms = tow_ms;
        cs->tow_at_preamble = tow_pre;
        cs->pll_180 = pll180;
        cs->valid_word = vw;
        cs->sent_tlm_failed = sent;
        cs->reserved = 0;
        cs->reserved2 = 0;
        a.counts[c] = count;
        a.faults[c] = fault ? 1 : 0;
    }
}

// reset() on one channel
__global__ void cnav_reset_kernel(gnsship_cnav_state* cs, int l5)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    cs->last_valid_preamble = cs->symbol_counter;
    cs->sent_tlm_failed = 0;
    if (l5) {
        cs->tow_ms = 0;
        cs->valid_word = 0;
    }
}

// A new block object: cnav_msg_decoder_init and zeroed members
void cnav_new_state(gnsship_cnav_state* st)
{
    *st = gnsship_cnav_state{};
    for (int k = 0; k < 2; k++) {
        for (int i = 1; i < 64; i++) st->part[k].metrics[0][i] = 63;  // v27_init: old_metrics = metrics1, state 0 biased
        st->part[k].init = 1;
    }
    st->part[1].symbols[0] = 0x80;  // cnav_add_symbol_(&dec->part2, 0x80)
    st->part[1].n_symbols = 1;
}

}  // namespace

struct gnsship_cnav {
    TlmHost h;  // h.mask: the output-valid flags
    gnsship_cnav_conf conf = {};
    int32_t messages_per_run = 0;
    gnsship_cnav_state* chans_dev = nullptr;
    gnsship_cnav_message* messages_dev = nullptr;
    int32_t* counts_dev = nullptr;
    uint8_t* faults_dev = nullptr;
    uint32_t* tow_dev = nullptr;
    uint8_t* sflags_dev = nullptr;
};

extern "C" int gnsship_cnav_destroy(gnsship_cnav* t)
{
    if (!t) return GNSSHIP_E_INVAL;
    t->h.release_all({t->chans_dev, t->messages_dev, t->counts_dev, t->faults_dev, t->tow_dev, t->sflags_dev});
    delete t;
    return GNSSHIP_OK;
}

extern "C" int gnsship_cnav_create(gnsship_ctx* ctx, const gnsship_cnav_conf* conf, int32_t max_channels, gnsship_cnav** out)
{
    if (!ctx || !out) return GNSSHIP_E_INVAL;
    *out = nullptr;
    if (!conf) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cnav_create: null configuration");
    if (conf->max_rounds < 1 || conf->max_rounds > GNSSHIP_CNAV_MAX_ROUNDS) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cnav_create: 1 <= max_rounds <= 2^20");
    if (conf->signal != GNSSHIP_CNAV_L2C && conf->signal != GNSSHIP_CNAV_L5) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cnav_create: signal must be GNSSHIP_CNAV_L2C or GNSSHIP_CNAV_L5");
    if (conf->reserved != 0) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cnav_create: reserved must be 0");
    if (max_channels < 1 || max_channels > GNSSHIP_CNAV_MAX_CHANNELS) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cnav_create: 1 <= max_channels <= 2^20");
    if (int rc = set_device(ctx)) return rc;
    gnsship_cnav* t = new (std::nothrow) gnsship_cnav();
    if (!t) return GNSSHIP_E_NOMEM;
    t->h.ctx = ctx;
    t->h.max_channels = max_channels;
    t->h.max_rounds = conf->max_rounds;
    t->conf = *conf;
    t->messages_per_run = GNSSHIP_CNAV_MESSAGES_PER_RUN(conf->max_rounds);
    const size_t nc = static_cast<size_t>(max_channels), slots = nc * t->messages_per_run, entries = nc * conf->max_rounds;
    hipError_t e = alloc_all(ctx, {dev_alloc(&t->chans_dev, nc, false), dev_alloc(&t->messages_dev, slots, true), dev_alloc(&t->counts_dev, nc, true),
                                      dev_alloc(&t->faults_dev, nc, true), dev_alloc(&t->tow_dev, entries, true), dev_alloc(&t->sflags_dev, entries, true)});
    if (e == hipSuccess) {  // every channel a new block object
        gnsship_cnav_state* fresh = new (std::nothrow) gnsship_cnav_state[nc];
        if (!fresh) {
            gnsship_cnav_destroy(t);
            return GNSSHIP_E_NOMEM;
        }
        for (size_t c = 0; c < nc; c++) cnav_new_state(fresh + c);
        e = hipMemcpyAsync(t->chans_dev, fresh, sizeof(gnsship_cnav_state) * nc, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // before `fresh` goes
        delete[] fresh;
    }
    if (e != hipSuccess) {
        gnsship_cnav_destroy(t);
        return hip_fail(ctx, e, "gnsship_cnav_create");
    }
    *out = t;
    return GNSSHIP_OK;
}

// Launch over n_rounds entries per channel already on the device, then copy what the caller wants.
static int cnav_launch(gnsship_cnav* t, const float* sym, const uint8_t* valid, const uint8_t* out_valid, const gnsship_trk_epoch* rec, int32_t n_rounds,
    gnsship_cnav_message* messages_host, int32_t* counts_host, uint8_t* faults_host, uint32_t* tow_ms_host, uint8_t* sflags_host, const char* who)
{
    gnsship_ctx* ctx = t->h.ctx;
    CnavArgs a = {};
    a.sym = sym;
    a.valid = valid;
    a.out_valid = out_valid;
    a.rec = rec;
    a.chans = t->chans_dev;
    a.messages = t->messages_dev;
    a.counts = t->counts_dev;
    a.faults = t->faults_dev;
    a.tow_ms = t->tow_dev;
    a.sflags = t->sflags_dev;
    a.max_channels = t->h.max_channels;
    a.n_rounds = n_rounds;
    a.messages_per_run = t->messages_per_run;
    a.signal = t->conf.signal;
    hipLaunchKernelGGL(cnav_kernel, dim3(static_cast<unsigned>(t->h.max_channels)), dim3(64), 0, ctx->stream, a);
    if (int rc = launched(ctx, who)) return rc;
    const size_t nc = static_cast<size_t>(t->h.max_channels), slots = nc * t->messages_per_run, entries = nc * n_rounds;
    return copy_out(ctx, {{messages_host, t->messages_dev, sizeof(gnsship_cnav_message) * slots}, {counts_host, t->counts_dev, sizeof(int32_t) * nc},
                                 {faults_host, t->faults_dev, nc}, {tow_ms_host, t->tow_dev, sizeof(uint32_t) * entries}, {sflags_host, t->sflags_dev, entries}}, who);
}

extern "C" int gnsship_cnav_run_symbols(gnsship_cnav* t, const float* symbols, const uint8_t* valid, const uint8_t* out_valid, int on_device,
    int32_t n_rounds, gnsship_cnav_message* messages_host, int32_t* counts_host, uint8_t* faults_host, uint32_t* tow_ms_host, uint8_t* sflags_host)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_cnav_run_symbols";
    if (int rc = tlm_symbols_in(t->h, who, on_device, n_rounds, &symbols, &valid, &out_valid)) return rc;
    return cnav_launch(t, symbols, valid, out_valid, nullptr, n_rounds, messages_host, counts_host, faults_host, tow_ms_host, sflags_host, who);
}

extern "C" int gnsship_cnav_run_records(gnsship_cnav* t, const gnsship_trk_epoch* records, int on_device, int32_t n_rounds,
    gnsship_cnav_message* messages_host, int32_t* counts_host, uint8_t* faults_host, uint32_t* tow_ms_host, uint8_t* sflags_host)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_cnav_run_records";
    if (int rc = tlm_records_in(t->h, who, on_device, n_rounds, &records)) return rc;
    return cnav_launch(t, nullptr, nullptr, nullptr, records, n_rounds, messages_host, counts_host, faults_host, tow_ms_host, sflags_host, who);
}

extern "C" int gnsship_cnav_run_trk(gnsship_cnav* t, gnsship_trk* trk, gnsship_cnav_message* messages_host, int32_t* counts_host, uint8_t* faults_host,
    uint32_t* tow_ms_host, uint8_t* sflags_host, int32_t* n_rounds_out)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_cnav_run_trk";
    const gnsship_trk_epoch* rec = nullptr;
    int32_t rounds = 0;
    if (int rc = tlm_trk_in(t->h, who, trk, &rec, &rounds)) return rc;
    if (n_rounds_out) *n_rounds_out = rounds;
    return cnav_launch(t, nullptr, nullptr, nullptr, rec, rounds, messages_host, counts_host, faults_host, tow_ms_host, sflags_host, who);
}

extern "C" int gnsship_cnav_outputs_device(gnsship_cnav* t, gnsship_cnav_message** messages, int32_t** counts, uint8_t** faults, uint32_t** tow_ms,
    uint8_t** sflags, int32_t* messages_per_run)
{
    if (!t) return GNSSHIP_E_INVAL;
    if (messages) *messages = t->messages_dev;
    if (counts) *counts = t->counts_dev;
    if (faults) *faults = t->faults_dev;
    if (tow_ms) *tow_ms = t->tow_dev;
    if (sflags) *sflags = t->sflags_dev;
    if (messages_per_run) *messages_per_run = t->messages_per_run;
    return GNSSHIP_OK;
}

extern "C" int gnsship_cnav_reset_channel(gnsship_cnav* t, int32_t channel)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_cnav_reset_channel";
    if (int rc = tlm_check_channel(t->h, who, channel)) return rc;
    if (int rc = set_device(t->h.ctx)) return rc;
    hipLaunchKernelGGL(cnav_reset_kernel, dim3(1), dim3(1), 0, t->h.ctx->stream, t->chans_dev + channel, t->conf.signal == GNSSHIP_CNAV_L5 ? 1 : 0);
    return launched(t->h.ctx, who);
}

// *st to the channel, through a staging copy so that the caller's memory is free when the call returns
static int cnav_put_state(gnsship_cnav* t, int32_t channel, const gnsship_cnav_state* st, const char* who)
{
    gnsship_ctx* ctx = t->h.ctx;
    hipError_t e = hipMemcpyAsync(t->chans_dev + channel, st, sizeof(*st), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e == hipSuccess ? GNSSHIP_OK : hip_fail(ctx, e, who);
}

extern "C" int gnsship_cnav_new_channel(gnsship_cnav* t, int32_t channel)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_cnav_new_channel";
    if (int rc = tlm_check_channel(t->h, who, channel)) return rc;
    if (int rc = set_device(t->h.ctx)) return rc;
    gnsship_cnav_state fresh;
    cnav_new_state(&fresh);
    return cnav_put_state(t, channel, &fresh, who);
}

extern "C" int gnsship_cnav_state_get(gnsship_cnav* t, int32_t channel, gnsship_cnav_state* st)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_cnav_state_get";
    if (int rc = tlm_check_state(t->h, who, channel, st)) return rc;
    if (int rc = set_device(t->h.ctx)) return rc;
    return copy_out(t->h.ctx, {{st, t->chans_dev + channel, sizeof(*st)}}, who);
}

extern "C" int gnsship_cnav_state_set(gnsship_cnav* t, int32_t channel, const gnsship_cnav_state* st)
{
    if (!t) return GNSSHIP_E_INVAL;
    gnsship_ctx* ctx = t->h.ctx;
    if (int rc = tlm_check_state(t->h, "gnsship_cnav_state_set", channel, st)) return rc;
    for (int k = 0; k < 2; k++) {
        const gnsship_cnav_part& p = st->part[k];
        const uint8_t flags[] = {p.old_is_metrics2, p.preamble_seen, p.invert, p.message_lock, p.crc_ok, p.init};
        for (uint8_t f : flags)
            if (f > 1) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cnav_state_set: a part's flags must be 0 or 1");
        if (p.n_symbols >= (p.init ? 128u : 64u)) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cnav_state_set: n_symbols must be below the part's decode threshold");
        if (p.n_decoded > static_cast<uint32_t>(kCnavMaxHeld)) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cnav_state_set: n_decoded <= 480");
        if (p.decisions_index >= 64u) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cnav_state_set: decisions_index < 64");
    }
    if (st->pll_180 > 1 || st->valid_word > 1 || st->sent_tlm_failed > 1) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_cnav_state_set: the block's flags must be 0 or 1");
    if (int rc = set_device(ctx)) return rc;
    return cnav_put_state(t, channel, st, "gnsship_cnav_state_set");
}
