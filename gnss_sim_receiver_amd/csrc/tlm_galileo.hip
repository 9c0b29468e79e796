// tlm_galileo.hip — the frame handling of galileo_telemetry_decoder_gs::general_work (galileo_telemetry_decoder_gs.cc
// :872-1094) on the device, for I/NAV, F/NAV and C/NAV frame geometry (include/gnsship.h, gnsship_tlm_*): symbol
// history, preamble correlation, the three-state frame-sync machine with its 180° flag, page-part extraction,
// de-interleave / G2 / Viterbi, even + odd assembly, CRC-24Q, the CRC-error counter, loss of sync and
// check_tlm_separation.  Input: floats with a validity mask, or tracking's epoch records (host, device, or in place
// where gnsship_trk left them).  Output: CRC-checked page parts and per-channel fault flags.
//
// Layout: one workgroup of one wavefront per channel.  A channel's symbols are strictly ordered and the machine's next
// step depends on the last page's CRC verdict, so one wave carries a channel through the whole run and decodes as many
// pages as fall due, which differs from channel to channel.  With one wave per workgroup no barrier is ever shared
// between waves: the __syncthreads below order this wave's own LDS and ring accesses and nothing else.
//   gather   lanes stride over the run's n_rounds entries of the channel, 64 at a time; a ballot of the valid entries
//            and a prefix popcount give each symbol its ordinal.
//   ring     the history is a ring of required + 1 floats per channel in HBM, channel-major; `wpos` is the next write
//            position, which is the oldest entry once the ring is full.
//   hits     states 0 / 1 only, full ring only: lane k forms the sign pattern of the P oldest entries as they stand after
//            the chunk's k-th symbol (the test is `< 0.0f`) — read before the chunk is appended, which is the same
//            thing: those P entries lie ahead of the k + 1 positions the chunk has written by then (k + 1 + P <= 80 <
//            required + 1) — and two ballots say all-match / all-mismatch.
//   machine  wave-uniform: states 0 / 1 walk the ballots with find-first-set, and a chunk is cut where the machine enters
//            state 2; state 2 jumps to the due symbol preamble_index + period and cuts the chunk there, so that the ring
//            holds exactly the symbols up to the due one when the frame is read.  check_tlm_separation is a comparison
//            against a bound that nothing but a good page moves, so one test per cut equals one per symbol.
//   decode   the frame from the ring (offset P from the oldest) through the 180° negation, the de-interleaver and the G2
//            flip into LDS, then the trellis and traceback vit_decode_kernel runs (vit_wave.h, shared), with the 64
//            carried metrics in a register for the whole run.
//   CRC-24Q  linear: lane i XORs bit i's remainder x^(n−1−i+24) mod g from a table built at create, the checksum bits
//            are XORed in at their own weights, a butterfly XOR joins the lanes: zero means the CRC holds.
// Every LDS and HBM index comes from lane numbers, sizes and ballot bits, never from a symbol's value.
// The host path around the kernel (staging, the run calls' checks, output copies) is tlm_host.h.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "tlm_device.h"
#include "tlm_host.h"
#include "vit_wave.h"

#pragma clang fp contract(off)

using namespace gnsship;

namespace {

constexpr int kTlmCrcErrorLimit = 6; // CRC_ERROR_LIMIT (:65)
constexpr uint32_t kCrc24qPoly = 0x1864CFBu;
constexpr int kTlmG0 = 121, kTlmG1 = 91;

struct TlmGeometry {
    const char* preamble;
    int32_t period, required, rows, cols, LL, crc_bits, max_without_valid;
};
const TlmGeometry kTlmGeometry[4] = {
    {"", 0, 0, 0, 0, 0, 0, 0},
    {"0101100000", 250, 510, 8, 30, 114, 196, 15000},
    {"101101110000", 500, 512, 8, 61, 238, 214, 2500},
    {"1011011101110000", 1000, 1016, 8, 123, 486, 462, 60000},
};

struct TlmChan {  // one block object's members, 64 bytes
    uint64_t symbol_counter, preamble_index, last_valid_preamble;
    uint64_t even_lo, even_hi;  // page_Even: bit i of the string at bit i
    int32_t stat, crc_error_counter, history_size, wpos;
    uint8_t pll_180, frame_sync, even_word_arrived, flag_crc_test, sent_tlm_failed, pad[3];
};
static_assert(sizeof(TlmChan) == 64, "TlmChan");

struct TlmArgs {
    const float* sym;              // n_rounds × max_channels, or null
    const uint8_t* valid;          // the same shape, or null
    const gnsship_trk_epoch* rec;  // the same shape, or null (then sym)
    TlmChan* chans;
    float* ring;                   // max_channels × cap
    float* sections;               // max_channels × 64
    gnsship_tlm_page* pages;       // max_channels × pages_per_run
    uint8_t* bits;                 // max_channels × pages_per_run × LL
    int32_t* counts;
    uint8_t* faults;
    const uint32_t* crc_table;     // crc_bits entries
    int32_t max_channels, n_rounds, pages_per_run;
    int32_t frame_type, P, period, cap, rows, cols, LL, crc_bits, max_without_valid;
    uint32_t pre_zero_mask;        // bit i: preamble[i] is '0' (−1)
};

// XOR over the wave, in every lane (all 64 lanes active)
__device__ __forceinline__ uint32_t tlm_wave_xor(uint32_t x)
{
    for (int d = 32; d >= 1; d >>= 1) x ^= static_cast<uint32_t>(__shfl_xor(static_cast<int>(x), d));
    return x;
}

// kFull: GNSSHIP_VIT_MODE_FULL
template <bool kFull>
__global__ __launch_bounds__(64) void tlm_kernel(const TlmArgs a)
{
    extern __shared__ ulonglong2 tlm_lds[];
    const int lane = threadIdx.x;
    const int c = blockIdx.x;  // the grid is max_channels workgroups
    const int T = a.LL + kVitTail, LL = a.LL, cap = a.cap, P = a.P, period = a.period;
    ulonglong2* surv = tlm_lds;  // per step: x decisions, y stored
    float* sym = reinterpret_cast<float*>(surv + T);
    uint8_t* obits = reinterpret_cast<uint8_t*>(sym);  // the symbols are dead once the trellis is through

    TlmChan* cs = a.chans + c;
    uint64_t counter = tlm_uniform64(cs->symbol_counter), preamble_index = tlm_uniform64(cs->preamble_index);
    uint64_t last_valid = tlm_uniform64(cs->last_valid_preamble);
    uint64_t even_lo = tlm_uniform64(cs->even_lo), even_hi = tlm_uniform64(cs->even_hi);
    int stat = tlm_uniform(cs->stat), crc_err = tlm_uniform(cs->crc_error_counter);
    int size = min(max(tlm_uniform(cs->history_size), 0), cap);
    int wpos = tlm_uniform(cs->wpos);
    wpos = (wpos < 0 || wpos >= cap) ? 0 : wpos;
    bool pll180 = tlm_uniform(cs->pll_180) != 0, frame_sync = tlm_uniform(cs->frame_sync) != 0;
    bool even_arrived = tlm_uniform(cs->even_word_arrived) != 0, flag_crc = tlm_uniform(cs->flag_crc_test) != 0;
    bool sent = tlm_uniform(cs->sent_tlm_failed) != 0;

    float* ring = a.ring + static_cast<size_t>(c) * cap;
    const int64_t sec = static_cast<int64_t>(c) * 64 + lane;
    float carried = kFull ? -kVitMaxLog : a.sections[sec];
    const uint32_t pre_one_mask = ~a.pre_zero_mask & ((1u << P) - 1u);

    int count = 0;
    bool fault = false;
    for (int base = 0; base < a.n_rounds; base += 64) {
        const int r = base + lane;
        bool v = r < a.n_rounds;
        float s = 0.0f;
        uint64_t sc = 0;
        if (v) {
            const size_t e = static_cast<size_t>(r) * a.max_channels + c;
            if (a.rec) {
                v = (a.rec[e].flags & 1) != 0;
                if (v) {
                    s = static_cast<float>(a.rec[e].prompt_i);
                    sc = a.rec[e].sample_counter;
                }
            } else {
                if (a.valid) v = a.valid[e] != 0;
                if (v) s = a.sym[e];
            }
        }
        const unsigned long long mask = __ballot(v);
        const int n = __popcll(mask);
        const int ord = __popcll(mask & ((1ull << lane) - 1ull));
        int done = 0;
        while (done < n) {
            int m = n - done;  // 1..64
            const bool was2 = stat == 2;
            if (was2) {
                const uint64_t left = preamble_index + static_cast<uint64_t>(period) - counter;  // >= 1 in state 2
                if (left < static_cast<uint64_t>(m)) m = static_cast<int>(max(left, static_cast<uint64_t>(1)));
            } else {
                bool hit_match = false, hit_mismatch = false;
                if (lane < m && size + lane + 1 >= cap) {  // full once this chunk's symbol `lane` is in
                    int p = wpos + lane + 1;
                    if (p >= cap) p -= cap;
                    uint32_t neg = 0;
                    for (int i = 0; i < P; i++) {
                        neg |= (ring[p] < 0.0f ? 1u : 0u) << i;
                        p = p + 1 == cap ? 0 : p + 1;
                    }
                    hit_match = neg == a.pre_zero_mask;
                    hit_mismatch = neg == pre_one_mask;
                }
                const unsigned long long mismatch = __ballot(hit_mismatch);
                unsigned long long hits = __ballot(hit_match) | mismatch;
                while (hits) {
                    const int j = __ffsll(hits) - 1;
                    hits &= hits - 1ull;
                    const uint64_t at = counter + static_cast<uint64_t>(j) + 1u;
                    if (stat == 0) {
                        preamble_index = at;
                        stat = 1;
                    } else {
                        const int32_t diff = static_cast<int32_t>(at - preamble_index);
                        if (diff == period) {
                            preamble_index = at;
                            crc_err = 0;
                            pll180 = (mismatch >> j) & 1ull;
                            stat = 2;
                            m = j + 1;
                            break;
                        }
                        if (diff > period) stat = 0;
                    }
                }
            }
            // append symbols done .. done + m − 1
            if (v && ord >= done && ord < done + m) {
                int p = wpos + (ord - done);
                if (p >= cap) p -= cap;
                ring[p] = s;
            }
            wpos += m;
            if (wpos >= cap) wpos -= cap;
            size = min(size + m, cap);
            counter += static_cast<uint64_t>(m);
            const int last_ord = done + m - 1;
            done += m;
            __syncthreads();  // the ring as it stands after these symbols, for this wave's reads below and next time round
            if (!sent && counter - last_valid > static_cast<uint64_t>(a.max_without_valid)) {  // check_tlm_separation
                sent = true;
                fault = true;
            }
            if (!(was2 && counter == preamble_index + static_cast<uint64_t>(period))) continue;

            // ---- a page part is due ----
            const int oldest = size == cap ? wpos : 0;
            for (int i = lane; i < 2 * T; i += 64) {  // P + 2·T = period <= cap: one wrap at most
                int p = oldest + P + i;
                if (p >= cap) p -= cap;
                float x = ring[p];
                const int j = vit_place(i, a.rows, a.cols, pll180, true, x);  // rows · cols == 2·T, so j < 2·T
                sym[j] = x;
            }
            __syncthreads();
            carried = vit_wave_trellis<kFull>(surv, sym, T, carried, lane, kTlmG0, kTlmG1);
            __syncthreads();
            if (lane == 0) vit_wave_traceback(surv, obits, T, LL);
            __syncthreads();

            const bool room = count < a.pages_per_run;
            const size_t slot = static_cast<size_t>(c) * a.pages_per_run + count;
            if (room)
                for (int i = lane; i < LL; i += 64) a.bits[slot * LL + i] = obits[i];

            // ---- decode_*_word after the decoder: page parts and CRC ----
            bool evaluated = false, odd = false;
            uint32_t x = 0;
            if (a.frame_type == GNSSHIP_TLM_INAV) {
                odd = obits[0] != 0;
                if (!odd) {
                    even_lo = __ballot(obits[lane] != 0);                           // LL = 114 > 63
                    even_hi = __ballot(lane + 64 < LL && obits[min(lane + 64, LL - 1)] != 0);
                    even_arrived = true;
                } else {
                    if (even_arrived) {
                        for (int i = lane; i < a.crc_bits; i += 64) {  // the joined string: even part, then this one
                            const bool b = i < LL ? ((i < 64 ? even_lo >> i : even_hi >> (i - 64)) & 1ull) != 0 : obits[i - LL] != 0;
                            if (b) x ^= a.crc_table[i];
                        }
                        if (lane < 24 && obits[a.crc_bits - LL + lane] != 0) x ^= 1u << (23 - lane);
                        evaluated = true;
                    }
                    even_arrived = false;
                }
            } else {
                for (int i = lane; i < a.crc_bits; i += 64)
                    if (obits[i] != 0) x ^= a.crc_table[i];
                if (lane < 24 && obits[a.crc_bits + lane] != 0) x ^= 1u << (23 - lane);
                evaluated = true;
            }
            x = tlm_wave_xor(x);
            if (evaluated) flag_crc = tlm_uniform(static_cast<int>(x)) == 0;
            const bool crc_ok = flag_crc;

            preamble_index = counter;
            bool lost = false;
            if (crc_ok) {
                crc_err = 0;
                last_valid = counter;
                frame_sync = true;
            } else {
                crc_err++;
                if (crc_err > kTlmCrcErrorLimit) {
                    frame_sync = false;
                    stat = 0;
                    lost = true;
                }
            }
            if (room) {
                // the completing entry's sample counter, from the lane that holds it
                const unsigned long long holder = __ballot(v && ord == last_ord);
                const int hl = holder ? __ffsll(holder) - 1 : 0;
                const uint32_t sc_lo = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(sc)), hl));
                const uint32_t sc_hi = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(sc >> 32)), hl));
                if (lane == 0) {
                    gnsship_tlm_page pg;
                    pg.symbol_counter = counter;
                    pg.sample_counter = (static_cast<uint64_t>(sc_hi) << 32) | sc_lo;
                    pg.channel = c;
                    pg.flags = (crc_ok ? 1 : 0) | (evaluated ? 2 : 0) | (pll180 ? 4 : 0) | (odd ? 8 : 0) | (frame_sync ? 16 : 0) | (lost ? 32 : 0);
                    pg.crc_error_counter = crc_err;
                    pg.pad = 0;
                    a.pages[slot] = pg;
                }
                count++;
            }
            __syncthreads();  // obits is read; the next frame may overwrite it
        }
    }

    if (!kFull) a.sections[sec] = carried;
    if (lane == 0) {
        TlmChan o;
        o.symbol_counter = counter;
        o.preamble_index = preamble_index;
        o.last_valid_preamble = last_valid;
        o.even_lo = even_lo;
        o.even_hi = even_hi;
        o.stat = stat;
        o.crc_error_counter = crc_err;
        o.history_size = size;
        o.wpos = wpos;
        o.pll_180 = pll180;
        o.frame_sync = frame_sync;
        o.even_word_arrived = even_arrived;
        o.flag_crc_test = flag_crc;
        o.sent_tlm_failed = sent;
        o.pad[0] = o.pad[1] = o.pad[2] = 0;
        *cs = o;
        a.counts[c] = count;
        a.faults[c] = fault ? 1 : 0;
    }
}

__global__ void tlm_fill_kernel(float* p, int64_t n, float v)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// reset() (what 1) and set_satellite() (what 0) on one channel
__global__ void tlm_control_kernel(TlmChan* cs, int what)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (what) {
        cs->frame_sync = 0;
        cs->stat = 0;
    }
    cs->last_valid_preamble = cs->symbol_counter;
    cs->sent_tlm_failed = 0;
}

}  // namespace

struct gnsship_tlm {
    TlmHost h;  // h.mask: unused
    gnsship_tlm_conf conf = {};
    TlmGeometry geo = {};
    int32_t P = 0, cap = 0, pages_per_run = 0;
    uint32_t pre_zero_mask = 0;
    TlmChan* chans_dev = nullptr;
    float* ring_dev = nullptr;
    float* sections_dev = nullptr;
    gnsship_tlm_page* pages_dev = nullptr;
    uint8_t* bits_dev = nullptr;
    int32_t* counts_dev = nullptr;
    uint8_t* faults_dev = nullptr;
    uint32_t* crc_dev = nullptr;
};

extern "C" int gnsship_tlm_destroy(gnsship_tlm* t)
{
    if (!t) return GNSSHIP_E_INVAL;
    t->h.release_all({t->chans_dev, t->ring_dev, t->sections_dev, t->pages_dev, t->bits_dev, t->counts_dev, t->faults_dev, t->crc_dev});
    delete t;
    return GNSSHIP_OK;
}

static int tlm_fill_sections(gnsship_tlm* t, int64_t first, int64_t n, const char* where)
{
    hipLaunchKernelGGL(tlm_fill_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, t->h.ctx->stream, t->sections_dev + first, n, -kVitMaxLog);
    return launched(t->h.ctx, where);
}

extern "C" int gnsship_tlm_create(gnsship_ctx* ctx, const gnsship_tlm_conf* conf, int32_t max_channels, gnsship_tlm** out)
{
    if (!ctx || !out) return GNSSHIP_E_INVAL;
    *out = nullptr;
    if (!conf) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_tlm_create: null configuration");
    if (conf->frame_type < GNSSHIP_TLM_INAV || conf->frame_type > GNSSHIP_TLM_CNAV)
        return fail(ctx, GNSSHIP_E_INVAL, "gnsship_tlm_create: frame_type must be GNSSHIP_TLM_INAV, _FNAV or _CNAV");
    if (conf->vit_mode != GNSSHIP_VIT_MODE_REFERENCE && conf->vit_mode != GNSSHIP_VIT_MODE_FULL)
        return fail(ctx, GNSSHIP_E_INVAL, "gnsship_tlm_create: unknown vit_mode");
    if (conf->max_rounds < 1 || conf->max_rounds > GNSSHIP_TLM_MAX_ROUNDS) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_tlm_create: 1 <= max_rounds <= 2^20");
    if (conf->reserved != 0) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_tlm_create: reserved must be 0");
    if (max_channels < 1 || max_channels > GNSSHIP_TLM_MAX_CHANNELS) return fail(ctx, GNSSHIP_E_INVAL, "gnsship_tlm_create: 1 <= max_channels <= 2^20");
    if (int rc = set_device(ctx)) return rc;
    gnsship_tlm* t = new (std::nothrow) gnsship_tlm();
    if (!t) return GNSSHIP_E_NOMEM;
    t->h.ctx = ctx;
    t->h.max_channels = max_channels;
    t->h.max_rounds = conf->max_rounds;
    t->conf = *conf;
    t->geo = kTlmGeometry[conf->frame_type];
    t->P = static_cast<int32_t>(std::strlen(t->geo.preamble));
    t->cap = t->geo.required + 1;
    t->pages_per_run = conf->max_rounds / t->geo.period + 1;
    for (int i = 0; i < t->P; i++)
        if (t->geo.preamble[i] == '0') t->pre_zero_mask |= 1u << i;
    // x^k mod g, k = 0 .. crc_bits + 23; bit i of an n-bit string contributes x^(n − 1 − i + 24)
    const int n = t->geo.crc_bits;
    std::vector<uint32_t> rem(static_cast<size_t>(n) + 24), table(static_cast<size_t>(n));
    uint32_t reg = 1;
    for (int k = 0; k < n + 24; k++) {
        rem[k] = reg;
        reg <<= 1;
        if (reg & 0x1000000u) reg ^= kCrc24qPoly;
        reg &= 0xFFFFFFu;
    }
    for (int i = 0; i < n; i++) table[i] = rem[n - 1 - i + 24];
    const size_t nc = static_cast<size_t>(max_channels), slots = nc * t->pages_per_run;
    hipError_t e = alloc_all(ctx, {dev_alloc(&t->chans_dev, nc, true), dev_alloc(&t->ring_dev, nc * t->cap, true), dev_alloc(&t->sections_dev, 64 * nc, false),
                                      dev_alloc(&t->pages_dev, slots, true), dev_alloc(&t->bits_dev, slots * t->geo.LL, true), dev_alloc(&t->counts_dev, nc, true),
                                      dev_alloc(&t->faults_dev, nc, true), dev_alloc(&t->crc_dev, static_cast<size_t>(n), false)});
    if (e == hipSuccess) e = hipMemcpyAsync(t->crc_dev, table.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // `table` is a local
    if (e != hipSuccess) {
        gnsship_tlm_destroy(t);
        return hip_fail(ctx, e, "gnsship_tlm_create");
    }
    if (int rc = tlm_fill_sections(t, 0, static_cast<int64_t>(max_channels) * 64, "gnsship_tlm_create(fill)")) {
        gnsship_tlm_destroy(t);
        return rc;
    }
    *out = t;
    return GNSSHIP_OK;
}

// Launch over n_rounds entries per channel already on the device, then copy what the caller wants.
static int tlm_launch(gnsship_tlm* t, const float* sym, const uint8_t* valid, const gnsship_trk_epoch* rec, int32_t n_rounds, gnsship_tlm_page* pages_host,
    uint8_t* bits_host, int32_t* counts_host, uint8_t* faults_host, const char* who)
{
    gnsship_ctx* ctx = t->h.ctx;
    TlmArgs a = {};
    a.sym = sym;
    a.valid = valid;
    a.rec = rec;
    a.chans = t->chans_dev;
    a.ring = t->ring_dev;
    a.sections = t->sections_dev;
    a.pages = t->pages_dev;
    a.bits = t->bits_dev;
    a.counts = t->counts_dev;
    a.faults = t->faults_dev;
    a.crc_table = t->crc_dev;
    a.max_channels = t->h.max_channels;
    a.n_rounds = n_rounds;
    a.pages_per_run = t->pages_per_run;
    a.frame_type = t->conf.frame_type;
    a.P = t->P;
    a.period = t->geo.period;
    a.cap = t->cap;
    a.rows = t->geo.rows;
    a.cols = t->geo.cols;
    a.LL = t->geo.LL;
    a.crc_bits = t->geo.crc_bits;
    a.max_without_valid = t->geo.max_without_valid;
    a.pre_zero_mask = t->pre_zero_mask;
    const size_t lds = 16 * static_cast<size_t>(vit_wave_lds_words(a.LL + kVitTail));  // 1.8 KiB I/NAV .. 11.6 KiB C/NAV
    if (t->conf.vit_mode == GNSSHIP_VIT_MODE_FULL)
        hipLaunchKernelGGL(tlm_kernel<true>, dim3(static_cast<unsigned>(t->h.max_channels)), dim3(64), lds, ctx->stream, a);
    else
        hipLaunchKernelGGL(tlm_kernel<false>, dim3(static_cast<unsigned>(t->h.max_channels)), dim3(64), lds, ctx->stream, a);
    if (int rc = launched(ctx, who)) return rc;
    const size_t nc = static_cast<size_t>(t->h.max_channels), slots = nc * t->pages_per_run;
    return copy_out(ctx, {{pages_host, t->pages_dev, sizeof(gnsship_tlm_page) * slots}, {bits_host, t->bits_dev, slots * t->geo.LL},
                                 {counts_host, t->counts_dev, sizeof(int32_t) * nc}, {faults_host, t->faults_dev, nc}}, who);
}

extern "C" int gnsship_tlm_run_symbols(gnsship_tlm* t, const float* symbols, const uint8_t* valid, int on_device, int32_t n_rounds,
    gnsship_tlm_page* pages_host, uint8_t* bits_host, int32_t* counts_host, uint8_t* faults_host)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_tlm_run_symbols";
    if (int rc = tlm_symbols_in(t->h, who, on_device, n_rounds, &symbols, &valid, nullptr)) return rc;
    return tlm_launch(t, symbols, valid, nullptr, n_rounds, pages_host, bits_host, counts_host, faults_host, who);
}

extern "C" int gnsship_tlm_run_records(gnsship_tlm* t, const gnsship_trk_epoch* records, int on_device, int32_t n_rounds, gnsship_tlm_page* pages_host,
    uint8_t* bits_host, int32_t* counts_host, uint8_t* faults_host)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_tlm_run_records";
    if (int rc = tlm_records_in(t->h, who, on_device, n_rounds, &records)) return rc;
    return tlm_launch(t, nullptr, nullptr, records, n_rounds, pages_host, bits_host, counts_host, faults_host, who);
}

extern "C" int gnsship_tlm_run_trk(gnsship_tlm* t, gnsship_trk* trk, gnsship_tlm_page* pages_host, uint8_t* bits_host, int32_t* counts_host,
    uint8_t* faults_host)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_tlm_run_trk";
    const gnsship_trk_epoch* rec = nullptr;
    int32_t rounds = 0;
    if (int rc = tlm_trk_in(t->h, who, trk, &rec, &rounds)) return rc;
    return tlm_launch(t, nullptr, nullptr, rec, rounds, pages_host, bits_host, counts_host, faults_host, who);
}

extern "C" int gnsship_tlm_outputs_device(gnsship_tlm* t, gnsship_tlm_page** pages, uint8_t** bits, int32_t** counts, uint8_t** faults,
    int32_t* pages_per_run)
{
    if (!t) return GNSSHIP_E_INVAL;
    if (pages) *pages = t->pages_dev;
    if (bits) *bits = t->bits_dev;
    if (counts) *counts = t->counts_dev;
    if (faults) *faults = t->faults_dev;
    if (pages_per_run) *pages_per_run = t->pages_per_run;
    return GNSSHIP_OK;
}

static int tlm_control(gnsship_tlm* t, int32_t channel, int what, const char* who)
{
    if (!t) return GNSSHIP_E_INVAL;
    if (int rc = tlm_check_channel(t->h, who, channel)) return rc;
    if (int rc = set_device(t->h.ctx)) return rc;
    hipLaunchKernelGGL(tlm_control_kernel, dim3(1), dim3(1), 0, t->h.ctx->stream, t->chans_dev + channel, what);
    return launched(t->h.ctx, who);
}

extern "C" int gnsship_tlm_reset_channel(gnsship_tlm* t, int32_t channel) { return tlm_control(t, channel, 1, "gnsship_tlm_reset_channel"); }

extern "C" int gnsship_tlm_set_satellite(gnsship_tlm* t, int32_t channel) { return tlm_control(t, channel, 0, "gnsship_tlm_set_satellite"); }

extern "C" int gnsship_tlm_new_channel(gnsship_tlm* t, int32_t channel)
{
    if (!t) return GNSSHIP_E_INVAL;
    gnsship_ctx* ctx = t->h.ctx;
    const char* who = "gnsship_tlm_new_channel";
    if (int rc = tlm_check_channel(t->h, who, channel)) return rc;
    if (int rc = set_device(ctx)) return rc;
    hipError_t e = hipMemsetAsync(t->chans_dev + channel, 0, sizeof(TlmChan), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->ring_dev + static_cast<size_t>(channel) * t->cap, 0, sizeof(float) * t->cap, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, who);
    return tlm_fill_sections(t, static_cast<int64_t>(channel) * 64, 64, who);
}

extern "C" int gnsship_tlm_state_get(gnsship_tlm* t, int32_t channel, gnsship_tlm_state* st)
{
    if (!t) return GNSSHIP_E_INVAL;
    const char* who = "gnsship_tlm_state_get";
    if (int rc = tlm_check_state(t->h, who, channel, st)) return rc;
    if (int rc = set_device(t->h.ctx)) return rc;
    TlmChan c;
    if (int rc = copy_out(t->h.ctx, {{&c, t->chans_dev + channel, sizeof(TlmChan)}}, who)) return rc;
    std::memset(st, 0, sizeof(*st));
    st->symbol_counter = c.symbol_counter;
    st->preamble_index = c.preamble_index;
    st->last_valid_preamble = c.last_valid_preamble;
    st->stat = c.stat;
    st->crc_error_counter = c.crc_error_counter;
    st->history_size = c.history_size;
    st->pll_180 = c.pll_180;
    st->frame_sync = c.frame_sync;
    st->even_word_arrived = c.even_word_arrived;
    st->flag_crc_test = c.flag_crc_test;
    st->sent_tlm_failed = c.sent_tlm_failed;
    return GNSSHIP_OK;
}
