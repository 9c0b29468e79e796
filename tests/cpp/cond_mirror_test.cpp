// The signal conditioner through the C++ mirror (include/gnsship_cpp.hpp Freq_Xlating_Fir_Filter_Hip):
// the adapter's property names and lowpass defaults, the accuracy contract against a float64 model
// written out here, call-split invariance, a two-band handle against single-band ones, and the device
// output handed to Pcps_Acquisition-style consumers as a device pointer (downloaded and compared).
// Prints one line per check; exit status 0 when all pass.  Needs a GPU.
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

int main()
{
    const double fs = 16000000.0;
    const int64_t n = 8000;
    std::vector<cf> x(static_cast<size_t>(n));
    uint32_t s = 12345U;
    for (auto& v : x) {
        s = s * 1664525U + 1013904223U;
        const float re = static_cast<float>(static_cast<int>(s >> 16) % 4001 - 2000) / 100.0F;
        s = s * 1664525U + 1013904223U;
        const float im = static_cast<float>(static_cast<int>(s >> 16) % 4001 - 2000) / 100.0F;
        v = cf(re, im);
    }
    try {
        gnsship::Freq_Xlating_Fir_Filter_Conf gps, bds;
        gps.IF = 4000000.0;
        gps.sampling_frequency = fs;
        gps.decimation_factor = 4;
        bds.IF = -4000000.0;
        bds.sampling_frequency = fs;
        bds.decimation_factor = 2;
        gnsship::Freq_Xlating_Fir_Filter_Hip one(gps, n), two({gps, bds}, n), other(bds, n);
        check(one.taps().size() == 193 && other.taps().size() == 97 && two.taps(1).size() == 97, "lowpass defaults: 193 and 97 taps");
        check(one.output_rate() == 4000000.0 && two.output_rate(1) == 8000000.0, "output rates");

        std::vector<cf> y(static_cast<size_t>(n / 4)), y2(static_cast<size_t>(n / 2));
        check(one.work(x.data(), n, y.data()) && one.n_out() == n / 4 && one.samples_in() == static_cast<uint64_t>(n), "work: one band");
        std::vector<cd> ref;
        std::vector<double> bound;
        model(x, one.taps(), 4, 4000000, 16000000, 0, ref, bound);
        const double r0 = contract_ratio(y, ref, bound, one.taps().size());
        std::printf("band +4 MHz, D 4: worst |err| / contract bound %.3f\n", r0);
        check(r0 <= 1.0, "accuracy contract, first sample 0");

        const uint64_t first = (1ULL << 31) + 12345ULL;
        check(one.reset(first), "reset(first_sample)");
        // the same stream in three calls
        std::vector<cf> ys(static_cast<size_t>(n / 4));
        const int64_t cuts[4] = {0, 4, 4004, n};
        bool ok = true;
        for (int c = 0; c < 3; c++) ok = ok && one.work(x.data() + cuts[c], cuts[c + 1] - cuts[c], ys.data() + cuts[c] / 4);
        check(ok && one.samples_in() == first + static_cast<uint64_t>(n), "work: three calls");
        model(x, one.taps(), 4, 4000000, 16000000, first, ref, bound);
        check(contract_ratio(ys, ref, bound, one.taps().size()) <= 1.0, "accuracy contract, first sample 2^31 + 12345");
        check(one.reset(first) && one.work(x.data(), n, y.data()) && std::memcmp(y.data(), ys.data(), sizeof(cf) * y.size()) == 0,
            "call-split invariance: bit-identical");

        // two bands in one handle == the single-band handles; outputs read back from the device pointers
        check(one.reset(0) && one.work(x.data(), n, y.data()) && other.work(x.data(), n, y2.data()), "single-band references");
        check(two.work(x.data(), GNSSHIP_FMT_CF32, false, n) && two.n_out(0) == n / 4 && two.n_out(1) == n / 2 && two.dev_out(0) && two.dev_out(1),
            "work: two bands, outputs left on the device");
        std::vector<cf> d0(y.size()), d1(y2.size());
        auto dev = gnsship::Device::get(0);
        gnsship_ctx_sync(dev->ctx());
        ok = gnsship_dev_download(dev->ctx(), d0.data(), two.dev_out(0), sizeof(cf) * d0.size()) == GNSSHIP_OK &&
             gnsship_dev_download(dev->ctx(), d1.data(), two.dev_out(1), sizeof(cf) * d1.size()) == GNSSHIP_OK;
        check(ok && std::memcmp(d0.data(), y.data(), sizeof(cf) * y.size()) == 0 && std::memcmp(d1.data(), y2.data(), sizeof(cf) * y2.size()) == 0,
            "two-band handle bit-identical to the single-band handles");

        check(!one.work(x.data(), 6, y.data()) && one.last_error().find("gnsship_cond_run") != std::string::npos, "n_in not a multiple of D rejected");
        bool threw = false;
        try {
            gnsship::Freq_Xlating_Fir_Filter_Conf bad = gps;
            bad.filter_type = "bandpass";
            gnsship::Freq_Xlating_Fir_Filter_Hip f(bad, n);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        check(threw, "filter_type bandpass without taps refused (pm_remez not restated)");
        threw = false;
        try {
            gnsship::Freq_Xlating_Fir_Filter_Conf bad = gps;
            bad.IF = 4000000.5;
            gnsship::Freq_Xlating_Fir_Filter_Hip f(bad, n);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        check(threw, "non-integer IF refused");
    } catch (const std::exception& e) {
        std::printf("FAIL: exception %s\n", e.what());
        return 2;
    }
    std::printf("%s\n", failures ? "cond_mirror_test FAILED" : "cond_mirror_test passed");
    return failures ? 1 : 0;
}
