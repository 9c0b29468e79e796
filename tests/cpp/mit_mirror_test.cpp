// The interference-mitigation mirrors (include/gnsship_cpp.hpp Pulse_Blanking_Filter_Hip, Notch_Filter_Hip,
// Notch_Filter_Lite_Hip).
//   mit_mirror_test defaults   prints the three *_Conf defaults and the coeff_rate -> n_segments_coeff derivation
//                              (no GPU; tests/test_cpp_mirror_mit.py compares them with the adapters' values)
//   mit_mirror_test            on the GPU: every class over a noise + tone / pulse stream, whole against cut into
//                              uneven runs (bit-identical), the two chain forms against each other, and the
//                              pulse-blanking adapter's IF path against the conditioner followed by the plain block.
// Prints one line per check; exit status 0 when all pass.
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gnsship_cpp.hpp"

using cf = std::complex<float>;

static int failures = 0;
static void check(bool ok, const char* what)
{
    std::printf("%s: %s\n", ok ? "ok" : "FAIL", what);
    if (!ok) failures++;
}

static int print_defaults()
{
    gnsship::Pulse_Blanking_Filter_Conf pb;
    gnsship::Notch_Filter_Conf nf;
    gnsship::Notch_Filter_Lite_Conf nl;
    std::printf("pulse_blanking pfa %.9g length %d segments_est %d segments_reset %d IF %.17g sampling_frequency %.17g bw %.17g tw %.17g\n", pb.pfa, pb.length,
        pb.segments_est, pb.segments_reset, pb.IF, pb.sampling_frequency, pb.bw, pb.tw);
    std::printf("notch pfa %.9g p_c_factor %.9g length %d segments_est %d segments_reset %d\n", nf.pfa, nf.p_c_factor, nf.length, nf.segments_est,
        nf.segments_reset);
    std::printf("notch_lite pfa %.9g p_c_factor %.9g length %d segments_est %d segments_reset %d sampling_frequency %.9g n_segments_coeff %d\n", nl.pfa,
        nl.p_c_factor, nl.length, nl.segments_est, nl.segments_reset, nl.sampling_frequency, nl.n_segments_coeff());
    const float cases[][3] = {{4000000.0F, 1000.0F, 32}, {50000000.0F, 12500.0F, 5}, {4000000.0F, 4000000.0F, 32}, {20480000.0F, 999.0F, 1024}};
    for (const auto& c : cases) {
        gnsship::Notch_Filter_Lite_Conf x;
        x.sampling_frequency = c[0];
        x.coeff_rate = c[1];
        x.length = static_cast<int>(c[2]);
        std::printf("coeff sampling_frequency %.9g coeff_rate %.9g length %d n_segments_coeff %d\n", x.sampling_frequency, x.coeff_rate, x.length,
            x.n_segments_coeff());
    }
    return 0;
}

static std::vector<cf> stream(size_t n, bool tone, bool pulses)
{
    std::mt19937 rng(12345);
    std::normal_distribution<float> g(0.0F, 1.0F);
    std::vector<cf> x(n);
    for (size_t i = 0; i < n; i++) {
        x[i] = cf(g(rng), g(rng));
        if (tone && (i / 3000) % 2 == 1) x[i] += 6.0F * cf(static_cast<float>(std::cos(0.4593 * i)), static_cast<float>(std::sin(0.4593 * i)));
        if (pulses && i % 1777 < 40) x[i] += cf(12.0F, -9.0F);
    }
    return x;
}

static bool same_bits(const std::vector<cf>& a, const std::vector<cf>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(cf)) == 0);
}

template <class F>
static std::vector<cf> run_cut(F& f, const std::vector<cf>& x, const std::vector<int64_t>& cuts)
{
    std::vector<cf> out, buf(x.size() + 2048);
    size_t pos = 0;
    for (size_t i = 0; i <= cuts.size(); i++) {
        const size_t n = i < cuts.size() ? std::min<size_t>(static_cast<size_t>(cuts[i]), x.size() - pos) : x.size() - pos;
        if (!f.work(x.data() + pos, false, static_cast<int64_t>(n), nullptr, buf.data())) {
            std::printf("work failed: %s\n", f.last_error().c_str());
            failures++;
            return out;
        }
        out.insert(out.end(), buf.begin(), buf.begin() + f.n_out());
        pos += n;
    }
    return out;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "defaults") == 0) return print_defaults();
    const size_t n = 20000;
    const std::vector<int64_t> cuts = {1, 31, 32, 33, 227, 0, 4096, 5};
    {
        gnsship::Notch_Filter_Conf c;
        c.segments_est = 8;
        c.segments_reset = 40;
        const std::vector<cf> x = stream(n, true, false);
        c.chain_form = GNSSHIP_MIT_CHAIN_SERIAL;
        gnsship::Notch_Filter_Hip serial(c, static_cast<int64_t>(n));
        c.chain_form = GNSSHIP_MIT_CHAIN_SPECULATIVE;
        gnsship::Notch_Filter_Hip spec(c, static_cast<int64_t>(n));
        const std::vector<cf> whole = run_cut(serial, x, {});
        check(whole.size() == (n - 1) / 32 * 32 && serial.state().pending_samples == static_cast<int64_t>(n - whole.size()), "Notch_Filter_Hip: emits the complete segments");
        check(same_bits(whole, run_cut(spec, x, {})), "Notch_Filter_Hip: speculative form bit-identical to the serial form");
        check(serial.reset(), "Notch_Filter_Hip: reset");
        check(same_bits(whole, run_cut(serial, x, cuts)), "Notch_Filter_Hip: cut into runs bit-identical to one run");
        bool differs = false;
        for (size_t i = 0; i < whole.size() && !differs; i++) differs = whole[i] != x[i + 1];
        check(differs && whole[0] == x[1], "Notch_Filter_Hip: copies with the block's one-sample advance, filters the tone");
    }
    {
        gnsship::Notch_Filter_Lite_Conf c;
        c.segments_est = 8;
        c.segments_reset = 40;
        c.coeff_rate = 4000000.0F / 96.0F;  // n_segments_coeff = 3
        const std::vector<cf> x = stream(n, true, false);
        gnsship::Notch_Filter_Lite_Hip f(c, static_cast<int64_t>(n));
        const std::vector<cf> whole = run_cut(f, x, {});
        check(c.n_segments_coeff() == 3 && whole.size() == n / 32 * 32 && whole[0] == x[0], "Notch_Filter_Lite_Hip: n_segments_coeff from coeff_rate, no advance");
        check(f.reset(), "Notch_Filter_Lite_Hip: reset");
        check(same_bits(whole, run_cut(f, x, cuts)), "Notch_Filter_Lite_Hip: cut into runs bit-identical to one run");
    }
    {
        gnsship::Pulse_Blanking_Filter_Conf c;
        c.segments_est = 8;
        c.segments_reset = 40;
        const std::vector<cf> x = stream(n, false, true);
        gnsship::Pulse_Blanking_Filter_Hip f(c, static_cast<int64_t>(n));
        const std::vector<cf> whole = run_cut(f, x, {});
        size_t zeros = 0;
        for (const cf& v : whole) zeros += v == cf(0, 0);
        check(!f.xlat() && whole.size() == n / 32 * 32 && zeros >= 32 && zeros % 32 == 0 && zeros < whole.size() / 2, "Pulse_Blanking_Filter_Hip: blanks whole segments");
        check(f.reset(), "Pulse_Blanking_Filter_Hip: reset");
        check(same_bits(whole, run_cut(f, x, cuts)), "Pulse_Blanking_Filter_Hip: cut into runs bit-identical to one run");
        // the IF path: the adapter's decimation-1 translating low-pass, then the block
        c.IF = 250000.0;
        gnsship::Pulse_Blanking_Filter_Hip fx(c, static_cast<int64_t>(n));
        const std::vector<cf> got = run_cut(fx, x, {});
        gnsship::Freq_Xlating_Fir_Filter_Conf xc;
        xc.IF = c.IF;
        xc.sampling_frequency = c.sampling_frequency;
        xc.bw = c.bw;
        xc.tw = c.bw / 10.0;
        gnsship::Freq_Xlating_Fir_Filter_Hip cond(xc, static_cast<int64_t>(n));
        std::vector<cf> mid(n);
        c.IF = 0.0;
        gnsship::Pulse_Blanking_Filter_Hip plain(c, static_cast<int64_t>(n));
        const bool ok = cond.work(x.data(), static_cast<int64_t>(n), mid.data());
        check(fx.xlat() && ok && same_bits(got, run_cut(plain, mid, {})), "Pulse_Blanking_Filter_Hip: IF path = Freq_Xlating_Fir_Filter_Hip (decimation 1) + the block");
    }
    std::printf(failures ? "mit_mirror_test FAILED (%d)\n" : "mit_mirror_test passed\n", failures);
    return failures ? 1 : 0;
}
