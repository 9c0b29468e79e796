// codes.cpp — product-side PRN replica generators (host C++), exported through the C ABI so the
// adapters can build the local codes they hand to the correlator / acquisition engines.
//
//  GPS L1 C/A   : G1 = 1 + x^3 + x^10, G2 = 1 + x^2 + x^3 + x^6 + x^8 + x^9 + x^10, PRN code =
//                 G1 ⊕ G2 delayed by the IS-GPS-200 delay  (reference gps_sdr_signal_replica.cc:25-110)
//  BeiDou B1I   : 11-stage Gold code, G2 output taps per PRN  (beidou_b1i_signal_replica.cc:26-110)
//  GPS L5I / L5Q : XA (13 stages, 1 + x^9 + x^10 + x^12 + x^13, short-cycled to 8190) ⊕ XB (13 stages,
//                 1 + x + x^3 + x^4 + x^6 + x^7 + x^8 + x^12 + x^13) advanced per PRN and component
//                 (IS-GPS-705 Table 3-Ia; reference gps_l5_signal_replica.cc:24-187); their sampled
//                 forms index the chips with ceil() in float (:193-298), unlike the L1 generators
//  BeiDou B3I   : G1 (13 stages, 1 + x + x^3 + x^4 + x^13, reset to all ones at 1111111111100) ⊕ G2 (13 stages,
//                 1 + x + x^5 + x^6 + x^7 + x^9 + x^10 + x^12 + x^13) started at a per-PRN phase
//                 (BDS-SIS-ICD-B3I; reference beidou_b3i_signal_replica.cc:26-165), sampled as B1I
//  GPS L2 CM     : 27-stage modular register, polynomial octal 0445112474, per-PRN initial state
//                 (IS-GPS-200 Table 3-IIa; reference gps_l2c_signal_replica.cc:25-39), sampled as L5Q
//  Galileo E5    : E5a-I / E5a-Q / E5b-I / E5b-Q primaries, 10230 chips: one 28-stage linear recurrence per component
//                 (the ICD's two 14-stage registers multiplied out; E5a-I and E5a-Q share theirs) from the PRN's
//                 first 28 chips (galileo_e5_tables.h; reference galileo_e5_signal_replica.cc:31-216 reads tables);
//                 sampled with resampler()'s truncating float index (gnss_signal_replica.cc:275-290)
//  GLONASS C/A  : one 9-stage maximal sequence (1 + x^5 + x^9, output stage 7), 511 chips, the same for every
//                 satellite and for L1 and L2 (glonass_l1_signal_replica.cc:25-123), sampled as B1I; the
//                 satellites differ by FDMA frequency channel (gnsship_glonass_freq_channel)
//  sampled forms: the Borre-style upsampling with a float chip clock and the last sample forced
//                 to the last chip  (gps_sdr_signal_replica.cc:145-185, beidou_b1i_signal_replica.cc:142-180)
//
// Registers are kept as integers (bit i = register cell i) instead of bitsets; outputs are identical,
// which tests/test_codes.py checks against the oracle and the golden fixtures.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "galileo_e5_tables.h"
#include "gnsship.h"

namespace e5 = gnsship::e5;

namespace {

// IS-GPS-200 G2 delays (chips) for PRN 1..210 (same table the reference carries at :41-51).
constexpr int16_t kGpsG2Delay[210] = {5, 6, 7, 8, 17, 18, 139, 140, 141, 251, 252, 254, 255, 256, 257, 258, 469, 470, 471, 472, 473, 474,
    509, 512, 513, 514, 515, 516, 859, 860, 861, 862, 863, 950, 947, 948, 950, 67, 103, 91, 19, 679, 225, 625, 946, 638, 161, 1001, 554,
    280, 710, 709, 775, 864, 558, 220, 397, 55, 898, 759, 367, 299, 1018, 729, 695, 780, 801, 788, 732, 34, 320, 327, 389, 407, 525, 405,
    221, 761, 260, 326, 955, 653, 699, 422, 188, 438, 959, 539, 879, 677, 586, 153, 792, 814, 446, 264, 1015, 278, 536, 819, 156, 957,
    159, 712, 885, 461, 248, 713, 126, 807, 279, 122, 197, 693, 632, 771, 467, 647, 203, 145, 175, 52, 21, 237, 235, 886, 657, 634, 762,
    355, 1012, 176, 603, 130, 359, 595, 68, 386, 797, 456, 499, 883, 307, 127, 211, 121, 118, 163, 628, 853, 484, 289, 811, 202, 1021,
    463, 568, 904, 670, 230, 911, 684, 309, 644, 932, 12, 314, 891, 212, 185, 675, 503, 150, 395, 345, 846, 798, 992, 357, 995, 877, 112,
    144, 476, 193, 109, 445, 291, 87, 399, 292, 901, 339, 208, 711, 189, 263, 537, 663, 942, 173, 900, 30, 500, 935, 556, 373, 85, 652, 310};

// Output sequence of a Fibonacci LFSR: state bit i is register cell i, cell 0 is the output and
// the register shifts towards cell 0; `fb_mask` selects the cells XORed into the new last cell.
template <int STAGES>
void lfsr_sequence(uint32_t state, uint32_t fb_mask, int len, uint8_t* out)
{
    for (int i = 0; i < len; i++) {
        out[i] = state & 1u;
        const uint32_t fb = __builtin_parity(state & fb_mask);
        state = (state >> 1) | (fb << (STAGES - 1));
    }
}

// BeiDou B1I G2 phase-selector taps (ICD stage numbers, stage k ↔ register cell 11-k; 0 = unused), PRN 1..63.
constexpr uint8_t kB1iTap[63][3] = {{1, 3, 0}, {1, 4, 0}, {1, 5, 0}, {1, 6, 0}, {1, 8, 0}, {1, 9, 0}, {1, 10, 0}, {1, 11, 0}, {2, 7, 0},
    {3, 4, 0}, {3, 5, 0}, {3, 6, 0}, {3, 8, 0}, {3, 9, 0}, {3, 10, 0}, {3, 11, 0}, {4, 5, 0}, {4, 6, 0}, {4, 8, 0}, {4, 9, 0}, {4, 10, 0},
    {4, 11, 0}, {5, 6, 0}, {5, 8, 0}, {5, 9, 0}, {5, 10, 0}, {5, 11, 0}, {6, 8, 0}, {6, 9, 0}, {6, 10, 0}, {6, 11, 0}, {8, 9, 0},
    {8, 10, 0}, {8, 11, 0}, {9, 10, 0}, {9, 11, 0}, {10, 11, 0}, {2, 7, 1}, {3, 4, 1}, {3, 6, 1}, {3, 8, 1}, {3, 10, 1}, {3, 11, 1},
    {4, 5, 1}, {4, 9, 1}, {5, 6, 1}, {5, 8, 1}, {5, 10, 1}, {5, 11, 1}, {6, 9, 1}, {8, 9, 1}, {9, 10, 1}, {9, 11, 1}, {3, 7, 2},
    {5, 7, 2}, {7, 9, 2}, {4, 5, 3}, {4, 9, 3}, {5, 6, 3}, {5, 8, 3}, {5, 10, 3}, {5, 11, 3}, {6, 9, 3}};

int gps_chips(int32_t prn, uint32_t chip_shift, int8_t* chips)
{
    if (prn < 1 || prn > 210) return GNSSHIP_E_INVAL;
    constexpr int L = 1023;
    uint8_t g1[L], g2[L];
    // cell i ↔ polynomial stage 10-i: G1 taps x^3,x^10 → cells 7,0; G2 taps x^2,x^3,x^6,x^8,x^9,x^10
    // → cells 8,7,4,2,1,0.  All-ones initial state.
    lfsr_sequence<10>(0x3FFu, (1u << 0) | (1u << 7), L, g1);
    lfsr_sequence<10>(0x3FFu, (1u << 0) | (1u << 1) | (1u << 2) | (1u << 4) | (1u << 7) | (1u << 8), L, g2);
    uint32_t d = (static_cast<uint32_t>(L - kGpsG2Delay[prn - 1]) + chip_shift) % L;
    for (int i = 0; i < L; i++) {
        chips[i] = (g1[(i + chip_shift) % L] ^ g2[d]) ? 1 : -1;
        d = (d + 1) % L;
    }
    return GNSSHIP_OK;
}

int b1i_chips(int32_t prn, uint32_t chip_shift, int8_t* chips)
{
    if (prn < 1 || prn > 63) return GNSSHIP_E_INVAL;
    constexpr int L = 2046;
    // initial phase 01010101010 (cell 0 = rightmost character of the string)
    constexpr uint32_t init = 0x2AAu;
    uint8_t g1[L], g2[L];
    lfsr_sequence<11>(init, 0x41Fu /* cells 0-4,10 */, L, g1);
    // G2: output = XOR of the selected stages of the current state; feedback cells 0,2,3,6,7,8,9,10
    uint32_t s = init;
    const uint8_t* tap = kB1iTap[prn - 1];
    for (int i = 0; i < L; i++) {
        uint32_t o = ((s >> (11 - tap[0])) ^ (s >> (11 - tap[1]))) & 1u;
        if (tap[2]) o ^= (s >> (11 - tap[2])) & 1u;
        g2[i] = static_cast<uint8_t>(o);
        const uint32_t fb = __builtin_parity(s & 0x7CDu);
        s = (s >> 1) | (fb << 10);
    }
    uint32_t d = chip_shift % L;
    for (int i = 0; i < L; i++) {
        chips[i] = (g1[(i + chip_shift) % L] ^ g2[d]) ? 1 : -1;
        d = (d + 1) % L;
    }
    return GNSSHIP_OK;
}

// IS-GPS-705 XB code advances (chips) of PRN 1..32: row 0 the I5 (data) component, row 1 the Q5 (pilot)
// component.  tests/test_codes_l5.py recovers each from the fixture chips (the unique shift at which
// XA ⊕ code equals the XB sequence).
constexpr int kL5Len = 10230;
constexpr int16_t kL5XbAdvance[2][32] = {
    {266, 365, 804, 1138, 1509, 1559, 1756, 2084, 2170, 2303, 2527, 2687, 2930, 3471, 3940, 4132, 4332, 4924, 5343, 5443, 5641, 5816, 5898,
        5918, 5955, 6243, 6345, 6477, 6518, 6875, 7168, 7187},
    {1701, 323, 5292, 2020, 5429, 7136, 1041, 5947, 4315, 148, 535, 1939, 5206, 5910, 3595, 5135, 6082, 6990, 3546, 1523, 4548, 4484, 1893,
        3961, 7106, 5299, 4660, 276, 4389, 3783, 1591, 1601}};

// component: 0 = L5I, 1 = L5Q.  Both share XA and XB (all-ones start); XA returns to all ones after the
// state 1111111111101 (cell 1 clear), i.e. every 8190 chips.
int l5_chips(int component, int32_t prn, int8_t* chips)
{
    if (prn < 1 || prn > 32) return GNSSHIP_E_INVAL;
    static uint8_t xa[kL5Len], xb[kL5Len];
    static const bool ready = [] {
        // cell i ↔ polynomial stage 13-i: XA taps 9,10,12,13 → cells 4,3,1,0
        uint32_t s = 0x1FFFu;
        for (int i = 0; i < kL5Len; i++) {
            xa[i] = s & 1u;
            s = s == 0x1FFDu ? 0x1FFFu : (s >> 1) | (static_cast<uint32_t>(__builtin_parity(s & 0x1Bu)) << 12);
        }
        // XB taps 1,3,4,6,7,8,12,13 → cells 12,10,9,7,6,5,1,0
        lfsr_sequence<13>(0x1FFFu, 0x16E3u, kL5Len, xb);
        return true;
    }();
    (void)ready;
    int d = kL5XbAdvance[component][prn - 1];
    for (int i = 0; i < kL5Len; i++) {
        chips[i] = (xa[i] ^ xb[d]) ? -1 : 1;  // 1 − 2·chip
        d = d + 1 == kL5Len ? 0 : d + 1;
    }
    return GNSSHIP_OK;
}

// The L5 generators' sampling rule (gps_l5_signal_replica.cc:193-226, :262-298): chip index
// (int)ceil(ts·(i + 1.0F)/tc) − 1 in float, the last sample forced to the last chip.  tc_double_div:
// L5I forms tc as 1.0 / float (:196), L5Q as 1.0F / float (:278).  An index past the last chip (the
// reference reads its array unchecked there) is held at the last chip.
int sample_code_ceil(const int8_t* chips, int code_len, int32_t chip_rate, int32_t fs, bool imag_part, bool tc_double_div, float* dest)
{
    if (fs <= 0) return GNSSHIP_E_INVAL;
    const float tc = tc_double_div ? static_cast<float>(1.0 / static_cast<double>(static_cast<float>(chip_rate)))
                                   : 1.0F / static_cast<float>(chip_rate);
    const float ts = 1.0F / static_cast<float>(fs);
    const auto n = static_cast<int32_t>(static_cast<double>(fs) / (static_cast<double>(chip_rate) / static_cast<double>(code_len)));
    for (int32_t i = 0; i < n; i++) {
        int32_t k = static_cast<int32_t>(std::ceil(ts * (static_cast<float>(i) + 1.0F) / tc)) - 1;
        if (i == n - 1 || k >= code_len) k = code_len - 1;
        if (k < 0) k = 0;
        const float v = static_cast<float>(chips[k]);
        dest[2 * i] = imag_part ? 0.0F : v;
        dest[2 * i + 1] = imag_part ? v : 0.0F;
    }
    return n;
}

// BeiDou B3I G2 register phase of PRN 1..63 (bit i = cell i, cell 0 the output), and the GPS L2 CM
// register's initial state of PRN 1..50 (bit 0 the output).  tests/test_codes_b3i_l2c.py recovers each from
// the fixture chips: G1 ⊕ code gives G2, whose first 13 outputs are its cells; the modular L2 CM
// register's output k depends on its bits 0..k only.
constexpr uint16_t kB3iG2Phase[63] = {0x15FF, 0x1E2B, 0x178A, 0x1FFB, 0x191F, 0x1264, 0x1FD2, 0x1DFD, 0x1402, 0x041B, 0x1D70, 0x059E,
    0x0C95, 0x0E26, 0x1189, 0x1C7C, 0x04C5, 0x00EC, 0x1157, 0x02DE, 0x042D, 0x058A, 0x02CF, 0x0662, 0x0748, 0x0929, 0x16D3, 0x15E2, 0x02F5,
    0x0FFF, 0x0D8F, 0x1589, 0x12AB, 0x19A5, 0x1A5D, 0x1F74, 0x0567, 0x1D10, 0x1B90, 0x1ACE, 0x1034, 0x0BD9, 0x0DBC, 0x1A71, 0x0722, 0x0AC5,
    0x13E6, 0x1F48, 0x0149, 0x10AC, 0x1E4C, 0x098F, 0x0018, 0x1004, 0x06A6, 0x1646, 0x0E78, 0x05CA, 0x19F6, 0x1245, 0x0E20, 0x0642, 0x044E};
constexpr uint32_t kL2cmInit[50] = {0x78A1FB4, 0x7B8181D, 0x00BCE64, 0x0D96BD4, 0x6060739, 0x70D35DB, 0x1529038, 0x63D9CF1, 0x09EC391,
    0x76C3226, 0x72E9465, 0x0523F86, 0x0456803, 0x2635AE9, 0x0059900, 0x2482346, 0x5816816, 0x216A3C5, 0x0D02464, 0x140E2BC, 0x090275B,
    0x753C8D7, 0x097C77F, 0x78503B0, 0x701785C, 0x0214EB1, 0x72E3725, 0x77DA872, 0x3272F1C, 0x7225407, 0x74A645B, 0x0A0F48B, 0x50357C3,
    0x7B47F1E, 0x17B9EF1, 0x7BB7B2B, 0x4768C4A, 0x7E5D7EB, 0x2588FC1, 0x0482A48, 0x40A6CE4, 0x7AAEC4C, 0x7081274, 0x0851DF9, 0x09E5EBD,
    0x2D9B674, 0x72CEEEE, 0x0C2CCDD, 0x3B4F61D, 0x63D021E};

int b3i_chips(int32_t prn, uint32_t chip_shift, int8_t* chips)
{
    if (prn < 1 || prn > 63) return GNSSHIP_E_INVAL;
    constexpr int L = kL5Len;
    static uint8_t g1[L];
    static const bool ready = [] {
        // G1: feedback cells 0, 9, 10, 12; back to all ones when the shifted register reads 1111111111100
        uint32_t s = 0x1FFFu;
        for (int i = 0; i < L; i++) {
            g1[i] = s & 1u;
            s = (s >> 1) | (static_cast<uint32_t>(__builtin_parity(s & 0x1601u)) << 12);
            if (s == 0x1FFCu) s = 0x1FFFu;
        }
        return true;
    }();
    (void)ready;
    static thread_local uint8_t g2[L];
    lfsr_sequence<13>(kB3iG2Phase[prn - 1], 0x11DBu /* cells 0,1,3,4,6,7,8,12 */, L, g2);
    uint32_t d = chip_shift % L;
    for (int i = 0; i < L; i++) {
        chips[i] = (g1[(i + chip_shift) % L] ^ g2[d]) ? 1 : -1;
        d = d + 1 == L ? 0 : d + 1;
    }
    return GNSSHIP_OK;
}

// PRN outside 1..50 is an error (the reference leaves the bits zero there: a code of all +1)
int l2cm_chips(int32_t prn, int8_t* chips)
{
    if (prn < 1 || prn > 50) return GNSSHIP_E_INVAL;
    uint32_t x = kL2cmInit[prn - 1];
    for (int i = 0; i < kL5Len; i++) {
        chips[i] = (x & 1u) ? -1 : 1;  // 1 − 2·bit
        x = (x >> 1) ^ ((x & 1u) * 0445112474u);
    }
    return GNSSHIP_OK;
}

// Borre upsampling (float chip clock), code value placed in re (imag_part=false) or im.
// tc_double_div: the B1I generator forms the chip period as 1.0 / float (a double division,
// beidou_b1i_signal_replica.cc:146), the GPS one as 1.0F / float (gps_sdr_signal_replica.cc:150).
int sample_code(const int8_t* chips, int code_len, int32_t chip_rate, int32_t fs, bool imag_part, bool tc_double_div, float* dest)
{
    if (fs <= 0) return GNSSHIP_E_INVAL;
    const float tc = tc_double_div ? static_cast<float>(1.0 / static_cast<double>(static_cast<float>(chip_rate)))
                                   : 1.0F / static_cast<float>(chip_rate);
    const float ts = 1.0F / static_cast<float>(fs);
    const auto n = static_cast<int32_t>(static_cast<double>(fs) / (static_cast<double>(chip_rate) / static_cast<double>(code_len)));
    for (int32_t i = 0; i < n; i++) {
        const float aux = (ts * (static_cast<float>(i) + 1)) / tc;
        int32_t k = static_cast<int32_t>(static_cast<int64_t>(aux + 1)) - 1;
        if (i == n - 1 || k >= code_len) k = code_len - 1;  // (past the last chip the reference reads its array unchecked)
        const float v = static_cast<float>(chips[k]);
        dest[2 * i] = imag_part ? 0.0F : v;
        dest[2 * i + 1] = imag_part ? v : 0.0F;
    }
    return n;
}

// Galileo E5a-I / E5a-Q / E5b-I / E5b-Q primary (component 0..3): chip n = parity of the previous 28 chips under
// the component's feedback mask, from the PRN's first 28 chips (galileo_e5_tables.h; the OS SIS ICD's two 14-stage
// registers multiplied out — one recurrence holds over the whole truncated code).  Bit 1 ↔ chip −1, as the
// reference's hex_to_binary_converter reads its tables (gnss_signal_replica.cc:43-146).
int e5_chips(int component, int32_t prn, int8_t* chips)
{
    if (prn < 1 || prn > 50 || component < 0 || component > 3) return GNSSHIP_E_INVAL;
    uint32_t w = e5::kStart[component][prn - 1];  // bit j = chip n − 28 + j
    const uint32_t fb = e5::kFeedback[component];
    for (int i = 0; i < e5::kStages; i++) chips[i] = ((w >> i) & 1u) ? -1 : 1;
    for (int i = e5::kStages; i < kL5Len; i++) {
        const uint32_t b = __builtin_parity(w & fb);
        w = (w >> 1) | (b << (e5::kStages - 1));
        chips[i] = b ? -1 : 1;
    }
    return GNSSHIP_OK;
}

// signal_id → first component (0 E5a-I .. 3 E5b-Q) and whether both components are asked for
bool e5_signal(const char* id, char band, int& component, bool& both)
{
    if (!id || id[0] != band || (id[1] != 'I' && id[1] != 'Q' && id[1] != 'X')) return false;
    component = (band == '5' ? 0 : 2) + (id[1] == 'Q' ? 1 : 0);
    both = id[1] == 'X';
    return true;
}

int e5_primary(float* dest, int32_t prn, const char* signal_id, char band)
{
    int comp;
    bool both;
    if (!dest || !e5_signal(signal_id, band, comp, both)) return GNSSHIP_E_INVAL;
    static thread_local int8_t re[kL5Len], im[kL5Len];
    if (int rc = e5_chips(comp, prn, re)) return rc;
    if (both)
        if (int rc = e5_chips(comp + 1, prn, im)) return rc;
    for (int i = 0; i < kL5Len; i++) {
        dest[2 * i] = static_cast<float>(re[i]);
        dest[2 * i + 1] = both ? static_cast<float>(im[i]) : 0.0F;
    }
    return GNSSHIP_OK;
}

// galileo_e5_a_code_gen_complex_sampled (galileo_e5_signal_replica.cc:96-122): resampler()'s index
// (gnss_signal_replica.cc:275-290) unless fs is the chip rate, then the delay rotation.  An index past the last
// chip (the reference reads its vector unchecked there) is held at the last chip.
int e5_sampled(float* dest, uint32_t prn, const char* signal_id, int32_t fs, uint32_t chip_shift, char band)
{
    if (!dest || fs <= 0) return GNSSHIP_E_INVAL;
    static thread_local float primary[2 * kL5Len];
    if (int rc = e5_primary(primary, static_cast<int32_t>(prn), signal_id, band)) return rc;
    constexpr uint32_t L = kL5Len;
    constexpr int32_t chip_rate = 10230000;
    const auto n = static_cast<uint32_t>(static_cast<double>(fs) / (static_cast<double>(chip_rate) / static_cast<double>(L)));
    if (n == 0) return GNSSHIP_E_INVAL;
    const uint32_t delay = ((L - chip_shift) % L) * n / L;
    const float fs_in = static_cast<float>(chip_rate), t_out = 1.0F / static_cast<float>(fs);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t k = i;
        if (fs != chip_rate) {
            const float aux = (t_out * (static_cast<float>(i) + 1.0F)) * fs_in;
            k = static_cast<uint32_t>(static_cast<int32_t>(static_cast<int64_t>(aux + 1)) - 1);
            if (i == n - 1 || k >= L) k = L - 1;
        }
        const uint32_t o = (i + delay) % n;
        dest[2 * o] = primary[2 * k];
        dest[2 * o + 1] = primary[2 * k + 1];
    }
    return static_cast<int>(n);
}

int e5_float(float* dest, int component, int32_t prn)
{
    if (!dest) return GNSSHIP_E_INVAL;
    static thread_local int8_t c[kL5Len];
    if (int rc = e5_chips(component, prn, c)) return rc;
    for (int i = 0; i < kL5Len; i++) dest[i] = static_cast<float>(c[i]);
    return GNSSHIP_OK;
}

int e5_q_secondary(char* dest, const uint32_t (*rows)[4], int count, int32_t prn)
{
    if (!dest || prn < 1 || prn > count) return GNSSHIP_E_INVAL;
    for (int i = 0; i < 100; i++) dest[i] = ((rows[prn - 1][i >> 5] >> (i & 31)) & 1u) ? '1' : '0';
    dest[100] = '\0';
    return GNSSHIP_OK;
}

}  // namespace

extern "C" int gnsship_galileo_e5_a_code_gen_complex_primary(float* dest, int32_t prn, const char* signal_id)
{
    return e5_primary(dest, prn, signal_id, '5');
}
extern "C" int gnsship_galileo_e5_b_code_gen_complex_primary(float* dest, int32_t prn, const char* signal_id)
{
    return e5_primary(dest, prn, signal_id, '7');
}
extern "C" int gnsship_galileo_e5_a_code_gen_complex_sampled(float* dest, uint32_t prn, const char* signal_id, int32_t fs, uint32_t chip_shift)
{
    return e5_sampled(dest, prn, signal_id, fs, chip_shift, '5');
}
extern "C" int gnsship_galileo_e5_b_code_gen_complex_sampled(float* dest, uint32_t prn, const char* signal_id, int32_t fs, uint32_t chip_shift)
{
    return e5_sampled(dest, prn, signal_id, fs, chip_shift, '7');
}
extern "C" int gnsship_galileo_e5a_i_code_gen_float(float* dest, int32_t prn) { return e5_float(dest, 0, prn); }
extern "C" int gnsship_galileo_e5a_q_code_gen_float(float* dest, int32_t prn) { return e5_float(dest, 1, prn); }
extern "C" int gnsship_galileo_e5b_i_code_gen_float(float* dest, int32_t prn) { return e5_float(dest, 2, prn); }
extern "C" int gnsship_galileo_e5b_q_code_gen_float(float* dest, int32_t prn) { return e5_float(dest, 3, prn); }
extern "C" int gnsship_galileo_e5a_i_secondary_code(char* dest)
{
    if (!dest) return GNSSHIP_E_INVAL;
    std::memcpy(dest, e5::kE5aISecondary, sizeof(e5::kE5aISecondary));
    return GNSSHIP_OK;
}
extern "C" int gnsship_galileo_e5b_i_secondary_code(char* dest)
{
    if (!dest) return GNSSHIP_E_INVAL;
    std::memcpy(dest, e5::kE5bISecondary, sizeof(e5::kE5bISecondary));
    return GNSSHIP_OK;
}
extern "C" int gnsship_galileo_e5a_q_secondary_code(char* dest, int32_t prn)
{
    return e5_q_secondary(dest, e5::kE5aQSecondary, e5::kE5aQSecondaryCount, prn);
}
extern "C" int gnsship_galileo_e5b_q_secondary_code(char* dest, int32_t prn) { return e5_q_secondary(dest, e5::kE5bQSecondary, 50, prn); }

extern "C" int gnsship_gps_l1_ca_code_gen_float(float* dest, int32_t prn, uint32_t chip_shift)
{
    if (!dest) return GNSSHIP_E_INVAL;
    int8_t c[1023];
    if (int rc = gps_chips(prn, chip_shift, c)) return rc;
    for (int i = 0; i < 1023; i++) dest[i] = static_cast<float>(c[i]);
    return GNSSHIP_OK;
}

extern "C" int gnsship_gps_l1_ca_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs, uint32_t chip_shift)
{
    if (!dest) return GNSSHIP_E_INVAL;
    int8_t c[1023];
    if (int rc = gps_chips(static_cast<int32_t>(prn), chip_shift, c)) return rc;
    return sample_code(c, 1023, 1023000, fs, true, false, dest);
}

extern "C" int gnsship_beidou_b1i_code_gen_float(float* dest, int32_t prn, uint32_t chip_shift)
{
    if (!dest) return GNSSHIP_E_INVAL;
    int8_t c[2046];
    if (int rc = b1i_chips(prn, chip_shift, c)) return rc;
    for (int i = 0; i < 2046; i++) dest[i] = static_cast<float>(c[i]);
    return GNSSHIP_OK;
}

extern "C" int gnsship_beidou_b1i_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs, uint32_t chip_shift)
{
    if (!dest) return GNSSHIP_E_INVAL;
    int8_t c[2046];
    if (int rc = b1i_chips(static_cast<int32_t>(prn), chip_shift, c)) return rc;
    return sample_code(c, 2046, 2046000, fs, false, true, dest);
}

static int l5_float(float* dest, int component, int32_t prn)
{
    if (!dest) return GNSSHIP_E_INVAL;
    static thread_local int8_t c[kL5Len];
    if (int rc = l5_chips(component, prn, c)) return rc;
    for (int i = 0; i < kL5Len; i++) dest[i] = static_cast<float>(c[i]);
    return GNSSHIP_OK;
}

extern "C" int gnsship_gps_l5i_code_gen_float(float* dest, int32_t prn) { return l5_float(dest, 0, prn); }
extern "C" int gnsship_gps_l5q_code_gen_float(float* dest, int32_t prn) { return l5_float(dest, 1, prn); }

extern "C" int gnsship_gps_l5i_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs)
{
    if (!dest) return GNSSHIP_E_INVAL;
    static thread_local int8_t c[kL5Len];
    if (int rc = l5_chips(0, static_cast<int32_t>(prn), c)) return rc;
    return sample_code_ceil(c, kL5Len, 10230000, fs, false, true, dest);
}

extern "C" int gnsship_gps_l5q_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs)
{
    if (!dest) return GNSSHIP_E_INVAL;
    static thread_local int8_t c[kL5Len];
    if (int rc = l5_chips(1, static_cast<int32_t>(prn), c)) return rc;
    return sample_code_ceil(c, kL5Len, 10230000, fs, true, false, dest);
}

extern "C" int gnsship_beidou_b3i_code_gen_float(float* dest, int32_t prn, uint32_t chip_shift)
{
    if (!dest) return GNSSHIP_E_INVAL;
    static thread_local int8_t c[kL5Len];
    if (int rc = b3i_chips(prn, chip_shift, c)) return rc;
    for (int i = 0; i < kL5Len; i++) dest[i] = static_cast<float>(c[i]);
    return GNSSHIP_OK;
}

extern "C" int gnsship_beidou_b3i_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs, uint32_t chip_shift)
{
    if (!dest) return GNSSHIP_E_INVAL;
    static thread_local int8_t c[kL5Len];
    if (int rc = b3i_chips(static_cast<int32_t>(prn), chip_shift, c)) return rc;
    return sample_code(c, kL5Len, 10230000, fs, false, true, dest);
}

extern "C" int gnsship_gps_l2c_m_code_gen_float(float* dest, int32_t prn)
{
    if (!dest) return GNSSHIP_E_INVAL;
    static thread_local int8_t c[kL5Len];
    if (int rc = l2cm_chips(prn, c)) return rc;
    for (int i = 0; i < kL5Len; i++) dest[i] = static_cast<float>(c[i]);
    return GNSSHIP_OK;
}

extern "C" int gnsship_gps_l2c_m_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs)
{
    if (!dest) return GNSSHIP_E_INVAL;
    static thread_local int8_t c[kL5Len];
    if (int rc = l2cm_chips(static_cast<int32_t>(prn), c)) return rc;
    return sample_code_ceil(c, kL5Len, 511500, fs, true, false, dest);
}

// GLONASS L1 / L2 C/A (glonass_l1_signal_replica.cc:25-77; the L2 generator is the same text): one 511-chip
// maximal sequence for every satellite.  Nine cells, all ones at the start; the output is cell 2 (the
// reference's G1_register[2], ICD stage 7 of 1 + x^5 + x^9), the feedback cells 4 ⊕ 0 enter at cell 8.
static void glonass_chips(uint32_t chip_shift, int8_t* chips)
{
    constexpr int L = 511;
    uint8_t g[L];
    uint32_t s = 0x1FFu;
    for (int i = 0; i < L; i++) {
        g[i] = (s >> 2) & 1u;
        const uint32_t fb = ((s >> 4) ^ s) & 1u;
        s = (s >> 1) | (fb << 8);
    }
    for (int i = 0; i < L; i++) chips[i] = g[(i + chip_shift) % L] ? 1 : -1;
}

extern "C" int gnsship_glonass_l1_ca_code_gen_float(float* dest, uint32_t chip_shift)
{
    if (!dest) return GNSSHIP_E_INVAL;
    int8_t c[511];
    glonass_chips(chip_shift, c);
    for (int i = 0; i < 511; i++) dest[i] = static_cast<float>(c[i]);
    return GNSSHIP_OK;
}

extern "C" int gnsship_glonass_l1_ca_code_gen_complex(float* dest, uint32_t chip_shift)
{
    if (!dest) return GNSSHIP_E_INVAL;
    int8_t c[511];
    glonass_chips(chip_shift, c);
    for (int i = 0; i < 511; i++) {
        dest[2 * i] = static_cast<float>(c[i]);
        dest[2 * i + 1] = 0.0F;
    }
    return GNSSHIP_OK;
}

// glonass_l1_ca_code_gen_complex_sampled (:83-123): tc = (float)(1.0 / (float)511000), the chip index
// ceil(ts·(i+1)/tc) − 1 in float, the last sample forced to the last chip — the B1I sampling rule.
extern "C" int gnsship_glonass_l1_ca_code_gen_complex_sampled(float* dest, int32_t fs, uint32_t chip_shift)
{
    if (!dest) return GNSSHIP_E_INVAL;
    int8_t c[511];
    glonass_chips(chip_shift, c);
    return sample_code(c, 511, 511000, fs, false, true, dest);
}

extern "C" int gnsship_glonass_l2_ca_code_gen_float(float* dest, uint32_t chip_shift) { return gnsship_glonass_l1_ca_code_gen_float(dest, chip_shift); }
extern "C" int gnsship_glonass_l2_ca_code_gen_complex(float* dest, uint32_t chip_shift)
{
    return gnsship_glonass_l1_ca_code_gen_complex(dest, chip_shift);
}
extern "C" int gnsship_glonass_l2_ca_code_gen_complex_sampled(float* dest, int32_t fs, uint32_t chip_shift)
{
    return gnsship_glonass_l1_ca_code_gen_complex_sampled(dest, fs, chip_shift);
}

// GLONASS_PRN (GLONASS_L1_L2_CA.h:134): the FDMA frequency channel k of orbital slot ("PRN") 0..24; entry 0
// is the reference's test entry.
extern "C" int gnsship_glonass_freq_channel(int32_t prn, int32_t* k)
{
    static constexpr int8_t kChannel[25] = {8, 1, -4, 5, 6, 1, -4, 5, 6, -2, -7, 0, -1, -2, -7, 0, -1, 4, -3, 3, -5, 4, -3, 3, 2};
    if (!k || prn < 0 || prn > 24) return GNSSHIP_E_INVAL;
    *k = kChannel[prn];
    return GNSSHIP_OK;
}

extern "C" int gnsship_code_samples_per_code(int32_t chip_rate, int32_t code_len, int32_t fs)
{
    if (chip_rate <= 0 || code_len <= 0 || fs <= 0) return GNSSHIP_E_INVAL;
    return static_cast<int32_t>(static_cast<double>(fs) / (static_cast<double>(chip_rate) / static_cast<double>(code_len)));
}
