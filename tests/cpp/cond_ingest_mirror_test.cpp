// The conditioner's real-sampled and bit-packed input items through the C++ mirror (include/gnsship_cpp.hpp):
// the source configurations' formats, Freq_Xlating_Fir_Filter_Conf::input_item_type, one real and one packed run
// against values computed here (a float64 model and an unpacker written out from the format's description), and a
// misaligned n_in refused.  Prints one line per check; exit status 0 when all pass.  The format checks need no GPU
// (`cond_ingest_mirror_test formats`); the runs do.
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gnsship_cpp.hpp"

using cf = std::complex<float>;
using cd = std::complex<double>;

static int failures = 0;
static void check(bool ok, const char* what)
{
    std::printf("%s: %s\n", ok ? "ok" : "FAIL", what);
    if (!ok) failures++;
}

// y[k] = sum_i h[i] x[kD - i] exp(-j 2 pi frac(fc (first + kD - i) / fs)) in double, and the bound sum |h||x|
static void model(const std::vector<cf>& x, const std::vector<float>& h, int D, int64_t fc, int64_t fs, uint64_t first, std::vector<cd>& y,
    std::vector<double>& bound)
{
    const int64_t n = static_cast<int64_t>(x.size());
    const int64_t fcm = ((fc % fs) + fs) % fs;
    y.assign(static_cast<size_t>(n / D), cd(0, 0));
    bound.assign(static_cast<size_t>(n / D), 0.0);
    for (int64_t k = 0; k < n / D; k++) {
        for (int64_t i = 0; i < static_cast<int64_t>(h.size()); i++) {
            const int64_t j = k * D - i;
            if (j < 0) break;
            const uint64_t r = (static_cast<uint64_t>(fcm) * ((first + static_cast<uint64_t>(j)) % static_cast<uint64_t>(fs))) % static_cast<uint64_t>(fs);
            const double a = 2.0 * M_PI * static_cast<double>(r) / static_cast<double>(fs);
            y[k] += static_cast<double>(h[i]) * cd(x[j]) * cd(std::cos(a), -std::sin(a));
            bound[k] += std::fabs(static_cast<double>(h[i])) * std::abs(cd(x[j]));
        }
    }
}

static double contract_ratio(const std::vector<cf>& y, const std::vector<cd>& ref, const std::vector<double>& bound, size_t T)
{
    double worst = 0.0;
    for (size_t k = 0; k < ref.size(); k++) {
        const double lim = (static_cast<double>(T) + 8.0) * std::ldexp(1.0, -23) * bound[k];
        const double err = std::abs(cd(y[k]) - ref[k]);
        if (lim == 0.0) {
            if (err != 0.0) return 1e30;
            continue;
        }
        worst = std::max(worst, err / lim);
    }
    return worst;
}

// bits-wide two's-complement field at bit offset off
static int field(uint8_t b, int off, int bits)
{
    int s = (b >> off) & ((1 << bits) - 1);
    return s >= (1 << (bits - 1)) ? s - (1 << bits) : s;
}

static void format_checks()
{
    using namespace gnsship;
    Two_Bit_Packed_File_Signal_Source_Conf tb;
    check(tb.sample_type == "real" && !tb.big_endian_bytes, "Two_Bit_Packed defaults: sample_type real, big_endian_bytes false");
    check(tb.format() == GNSSHIP_FMT_PACKED(2, GNSSHIP_FMT_PACKED_REAL, GNSSHIP_FMT_PACKED_LSB_FIRST, GNSSHIP_FMT_PACKED_MAP_2S1),
        "Two_Bit_Packed real: 2 bits, REAL, LSB first, 2s+1");
    tb.big_endian_bytes = true;
    tb.sample_type = "qi";
    check(tb.format() == GNSSHIP_FMT_PACKED(2, GNSSHIP_FMT_PACKED_QI, GNSSHIP_FMT_PACKED_MSB_FIRST, GNSSHIP_FMT_PACKED_MAP_2S1),
        "Two_Bit_Packed qi, big_endian_bytes: QI, MSB first");
    tb.sample_type = "iq";
    check(tb.format() == Two_Bit_Cpx_File_Signal_Source_Conf().format(), "Two_Bit_Packed iq, big_endian_bytes is Two_Bit_Cpx's layout");
    tb.sample_type = "complex";
    check(tb.format() == -1, "Two_Bit_Packed: unknown sample_type has no format");
    check(Nsr_File_Signal_Source_Conf().format() == GNSSHIP_FMT_PACKED(2, GNSSHIP_FMT_PACKED_REAL, GNSSHIP_FMT_PACKED_LSB_FIRST, GNSSHIP_FMT_PACKED_MAP_S),
        "Nsr: 2 bits, REAL, LSB first, s");
    check(Two_Bit_Cpx_File_Signal_Source_Conf().format() ==
              GNSSHIP_FMT_PACKED(2, GNSSHIP_FMT_PACKED_IQ, GNSSHIP_FMT_PACKED_MSB_FIRST, GNSSHIP_FMT_PACKED_MAP_2S1),
        "Two_Bit_Cpx: 2 bits, IQ, MSB first, 2s+1");
    Four_Bit_Cpx_File_Signal_Source_Conf fb;
    check(fb.sample_type == "iq" && fb.format() == GNSSHIP_FMT_PACKED(4, GNSSHIP_FMT_PACKED_IQ, GNSSHIP_FMT_PACKED_LSB_FIRST, GNSSHIP_FMT_PACKED_MAP_2S1),
        "Four_Bit_Cpx default iq: 4 bits, IQ, LSB first, 2s+1");
    fb.sample_type = "qi";
    check(fb.format() == GNSSHIP_FMT_PACKED(4, GNSSHIP_FMT_PACKED_QI, GNSSHIP_FMT_PACKED_LSB_FIRST, GNSSHIP_FMT_PACKED_MAP_2S1), "Four_Bit_Cpx qi");
    fb.sample_type = "real";
    check(fb.format() == -1, "Four_Bit_Cpx: sample_type real has no format");

    Freq_Xlating_Fir_Filter_Conf c;
    check(c.input_item_type == "gr_complex" && c.input_format() == GNSSHIP_FMT_CF32, "input_item_type default gr_complex");
    c.input_item_type = "float";
    check(c.input_format() == GNSSHIP_FMT_RF32, "input_item_type float");
    c.input_item_type = "short";
    check(c.input_format() == GNSSHIP_FMT_RI16, "input_item_type short");
    c.input_item_type = "byte";
    check(c.input_format() == GNSSHIP_FMT_RI8, "input_item_type byte");
    c.input_item_type = "cshort";
    check(c.input_format() == -1, "input_item_type cshort is not an input of the adapter");

    const int all[] = {GNSSHIP_FMT_CF32, GNSSHIP_FMT_CI16, GNSSHIP_FMT_CI8, GNSSHIP_FMT_RF32, GNSSHIP_FMT_RI16, GNSSHIP_FMT_RI8,
        GNSSHIP_FMT_NSR, GNSSHIP_FMT_TWO_BIT_CPX, GNSSHIP_FMT_FOUR_BIT_CPX(GNSSHIP_FMT_PACKED_IQ)};
    const int bits[] = {64, 32, 16, 32, 16, 8, 2, 4, 8};
    bool ok = true;
    for (int i = 0; i < 9; i++) ok = ok && gnsship_cond_fmt_bits(all[i]) == bits[i];
    for (int i = 0; i < 9; i++)
        for (int j = i + 1; j < 9; j++) ok = ok && all[i] != all[j];
    check(ok && gnsship_cond_fmt_bits(6) == 0 && gnsship_cond_fmt_bits(0x100) == 0, "format values disjoint, bits per sample");
}

int main(int argc, char** argv)
{
    format_checks();
    if (argc > 1 && std::strcmp(argv[1], "formats") == 0) {
        std::printf("%s\n", failures ? "cond_ingest_mirror_test FAILED" : "cond_ingest_mirror_test formats passed");
        return failures ? 1 : 0;
    }
    const double fs = 16000000.0;
    const int64_t n = 8000;
    // a real int16 stream and a byte stream (n / 4 bytes of 2-bit real items, n bytes of 4-bit complex items)
    std::vector<int16_t> xr(static_cast<size_t>(n));
    std::vector<uint8_t> bytes(static_cast<size_t>(n));
    uint32_t s = 2024U;
    for (auto& v : xr) {
        s = s * 1664525U + 1013904223U;
        v = static_cast<int16_t>(static_cast<int>(s >> 16) % 4001 - 2000);
    }
    for (auto& v : bytes) {
        s = s * 1664525U + 1013904223U;
        v = static_cast<uint8_t>(s >> 24);
    }
    try {
        gnsship::Freq_Xlating_Fir_Filter_Conf conf;
        conf.IF = 4000000.0;
        conf.sampling_frequency = fs;
        conf.decimation_factor = 4;
        conf.input_item_type = "short";
        gnsship::Freq_Xlating_Fir_Filter_Hip real_filter(conf, n);
        check(real_filter.taps().size() == 193 && real_filter.input_format() == GNSSHIP_FMT_RI16, "input_item_type short: a real int16 stream");

        std::vector<cf> y(static_cast<size_t>(n / 4)), x(static_cast<size_t>(n));
        std::complex<float>* ho[1] = {y.data()};
        std::vector<cd> ref;
        std::vector<double> bound;
        const uint64_t first = (1ULL << 31) + 12345ULL;
        for (int64_t i = 0; i < n; i++) x[static_cast<size_t>(i)] = cf(static_cast<float>(xr[static_cast<size_t>(i)]), 0.0F);
        check(real_filter.reset(first) && real_filter.work_items(xr.data(), false, n, nullptr, ho) && real_filter.n_out() == n / 4, "work: real short items");
        model(x, real_filter.taps(), 4, 4000000, 16000000, first, ref, bound);
        double r = contract_ratio(y, ref, bound, real_filter.taps().size());
        std::printf("real short items: worst |err| / contract bound %.3f\n", r);
        check(r <= 1.0, "accuracy contract, real short items");

        conf.input_item_type = "gr_complex";
        gnsship::Freq_Xlating_Fir_Filter_Hip filter(conf, n);
        // Two_Bit_Packed real, big_endian_bytes: field j at bit offset 6 - 2j, value 2s + 1
        gnsship::Two_Bit_Packed_File_Signal_Source_Conf tb;
        tb.big_endian_bytes = true;
        for (int64_t i = 0; i < n; i++)
            x[static_cast<size_t>(i)] = cf(static_cast<float>(2 * field(bytes[static_cast<size_t>(i / 4)], 6 - 2 * static_cast<int>(i % 4), 2) + 1), 0.0F);
        check(filter.reset(first) && filter.work(bytes.data(), tb.format(), false, n, nullptr, ho), "work: Two_Bit_Packed real, big_endian_bytes");
        model(x, filter.taps(), 4, 4000000, 16000000, first, ref, bound);
        r = contract_ratio(y, ref, bound, filter.taps().size());
        std::printf("Two_Bit_Packed real items: worst |err| / contract bound %.3f\n", r);
        check(r <= 1.0, "accuracy contract, Two_Bit_Packed real items");
        // the same stream in three calls cut inside the filter's history, bit-identical
        std::vector<cf> ys(static_cast<size_t>(n / 4));
        const int64_t cuts[4] = {0, 4, 4004, n};
        bool ok = filter.reset(first);
        for (int c = 0; c < 3; c++) {
            std::complex<float>* hs[1] = {ys.data() + cuts[c] / 4};
            ok = ok && filter.work(bytes.data() + cuts[c] / 4, tb.format(), false, cuts[c + 1] - cuts[c], nullptr, hs);
        }
        check(ok && std::memcmp(y.data(), ys.data(), sizeof(cf) * y.size()) == 0, "Two_Bit_Packed: three calls bit-identical to one");

        // Four_Bit_Cpx qi: low nibble = im, high nibble = re, value 2s + 1
        gnsship::Four_Bit_Cpx_File_Signal_Source_Conf fb;
        fb.sample_type = "qi";
        for (int64_t i = 0; i < n; i++) {
            const uint8_t b = bytes[static_cast<size_t>(i)];
            x[static_cast<size_t>(i)] = cf(static_cast<float>(2 * field(b, 4, 4) + 1), static_cast<float>(2 * field(b, 0, 4) + 1));
        }
        check(filter.reset(0) && filter.work(bytes.data(), fb.format(), false, n, nullptr, ho), "work: Four_Bit_Cpx qi");
        model(x, filter.taps(), 4, 4000000, 16000000, 0, ref, bound);
        r = contract_ratio(y, ref, bound, filter.taps().size());
        std::printf("Four_Bit_Cpx qi items: worst |err| / contract bound %.3f\n", r);
        check(r <= 1.0, "accuracy contract, Four_Bit_Cpx qi items");

        // n_in a multiple of D = 4 but not of lcm(D, samples per byte): D = 2 with 2-bit real items
        conf.decimation_factor = 2;
        gnsship::Freq_Xlating_Fir_Filter_Hip half(conf, n);
        const uint64_t before = half.samples_in();
        check(!half.work(bytes.data(), tb.format(), false, 10, nullptr, nullptr) && half.last_error().find("samples per byte") != std::string::npos &&
                  half.samples_in() == before,
            "n_in not a multiple of the samples per byte refused, stream untouched");
        check(half.work(bytes.data(), tb.format(), false, 12, nullptr, nullptr) && half.samples_in() == before + 12, "the next aligned run goes through");
        bool threw = false;
        try {
            gnsship::Freq_Xlating_Fir_Filter_Conf bad = conf;
            bad.input_item_type = "cbyte";
            gnsship::Freq_Xlating_Fir_Filter_Hip f(bad, n);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        check(threw, "unknown input_item_type refused");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "cond_ingest_mirror_test FAILED" : "cond_ingest_mirror_test passed");
    return failures ? 1 : 0;
}
