// glonass_mirror_test — GLONASS L1 / L2 C/A acquisition through the C++ mirror (include/gnsship_cpp.hpp).
//
//   glonass_mirror_test conf OUT.bin
//       the mirror's generators under the reference's names, written as raw floats: the 511 complex chips at
//       chip_shift 3, then the L2 code sampled at 6.625 Msps.  Then, as text on stdout: the derived sizes of
//       glonass_l1_ca_acq_conf / glonass_l2_ca_acq_conf at 6.625 Msps with sampled_ms 2, and for PRN 0..24 the
//       frequency channel and is_fdma()'s bias on "1G" and "2G", and the tracking adapters' configuration from
//       glonass_l1_ca_trk_conf / glonass_l2_ca_trk_conf.  PRN 25 must be refused.  Needs no device.
//
//   glonass_mirror_test acq IF.bin FS PRN K0 K1 ...
//       Pcps_Acquisition_Hip over the first 1 ms of an IF file (gr_complex): the FDMA sweep over the frequency
//       channels K0 K1 ... ("1G"), one line per channel, then the block's own grid for PRN with the bias
//       set_gnss_synchro("1G", PRN) applies, one line.  A line: doppler_hz delay_samples test_statistic positive.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gnsship_cpp.hpp"

static int conf_mode(const char* path)
{
    std::vector<std::complex<float>> chips(511), sampled(6625);
    gnsship::glonass_l1_ca_code_gen_complex(chips.data(), 3);
    if (gnsship::glonass_l2_ca_code_gen_complex_sampled(sampled.data(), 6625000, 0) != 6625) return 1;
    std::FILE* o = std::fopen(path, "wb");
    if (!o || std::fwrite(chips.data(), sizeof(chips[0]), chips.size(), o) != chips.size() ||
        std::fwrite(sampled.data(), sizeof(sampled[0]), sampled.size(), o) != sampled.size() || std::fclose(o) != 0) {
        std::fprintf(stderr, "cannot write %s\n", path);
        return 2;
    }
    gnsship::Acq_Conf in;
    in.fs_in = 6625000;
    in.sampled_ms = 2;
    in.use_automatic_resampler = true;  // never designs one: the optimum rate is 100e6
    in.chips_per_second = 1;            // overwritten by the helpers
    for (int band = 1; band <= 2; band++) {
        const gnsship::Acq_Conf c = band == 1 ? gnsship::glonass_l1_ca_acq_conf(in) : gnsship::glonass_l2_ca_acq_conf(in);
        const auto code = band == 1 ? gnsship::glonass_l1_ca_acquisition_code(c) : gnsship::glonass_l2_ca_acquisition_code(c);
        bool copies = code.size() == 13250;
        for (size_t i = 0; copies && i < 6625; i++) copies = code[i] == sampled[i] && code[6625 + i] == sampled[i];
        std::printf("conf %d ms_per_code %u chips_per_second %u samples_per_chip %u samples_per_code %.1f resampled_fs %lld ratio %.1f code %zu copies %d\n",
            band, c.ms_per_code, c.chips_per_second, c.samples_per_chip, static_cast<double>(c.samples_per_code),
            static_cast<long long>(c.resampled_fs), static_cast<double>(c.resampler_ratio), code.size(), copies ? 1 : 0);
    }
    for (uint32_t prn = 0; prn <= 24; prn++) {
        int32_t k = 99;
        if (!gnsship::glonass_freq_channel(prn, &k)) return 1;
        std::printf("prn %u k %d bias1 %d bias2 %d\n", prn, k, gnsship::glonass_doppler_bias_hz("1G", k), gnsship::glonass_doppler_bias_hz("2G", k));
    }
    gnsship::Dll_Pll_Conf tin;
    tin.fs_in = 6625000.0;
    tin.if_hz = 1000.0;
    for (int band = 1; band <= 2; band++) {
        const gnsship::Dll_Pll_Conf t = band == 1 ? gnsship::glonass_l1_ca_trk_conf(tin) : gnsship::glonass_l2_ca_trk_conf(tin);
        std::printf("trk %d system %c signal %s pll %.1f dll %.1f spacing %.2f vector_length %u max_lock_fail %d pilot %d rotator %d if %.1f\n", band,
            t.system, t.signal, static_cast<double>(t.pll_bw_hz), static_cast<double>(t.dll_bw_hz), static_cast<double>(t.early_late_space_chips),
            t.vector_length, t.max_carrier_lock_fail, t.track_pilot ? 1 : 0, t.rotator, t.if_hz);
    }
    int32_t k = 0;
    if (gnsship::glonass_freq_channel(25, &k)) {
        std::fprintf(stderr, "PRN 25 was accepted\n");
        return 1;
    }
    std::printf("PRN 25 refused\n");
    return 0;
}

static void print(const gnsship::Acq_Outcome& o)
{
    std::printf("%.1f %.17g %.9g %d\n", o.Acq_doppler_hz, o.Acq_delay_samples, static_cast<double>(o.test_statistics), o.positive ? 1 : 0);
}

int main(int argc, char** argv)
{
    if (argc == 3 && std::strcmp(argv[1], "conf") == 0) return conf_mode(argv[2]);
    if (argc < 6 || std::strcmp(argv[1], "acq") != 0) {
        std::fprintf(stderr, "usage: glonass_mirror_test conf OUT.bin\n       glonass_mirror_test acq IF.bin FS PRN K0 [K1 ...]\n");
        return 2;
    }
    gnsship::Acq_Conf in;
    in.fs_in = std::atoll(argv[3]);
    in.doppler_max = 5000;
    in.doppler_step = 500.0F;
    in.pfa = 1e-6F;
    const gnsship::Acq_Conf conf = gnsship::glonass_l1_ca_acq_conf(in);
    const uint32_t prn = static_cast<uint32_t>(std::atoi(argv[4]));
    std::vector<int32_t> bias;
    for (int i = 5; i < argc; i++) bias.push_back(gnsship::glonass_doppler_bias_hz("1G", std::atoi(argv[i])));
    try {
        gnsship::Pcps_Acquisition_Hip acq(conf);
        std::vector<std::complex<float>> x(static_cast<size_t>(acq.consumed_samples()));
        std::FILE* f = std::fopen(argv[2], "rb");
        if (!f || std::fread(x.data(), sizeof(x[0]), x.size(), f) != x.size()) {
            std::fprintf(stderr, "cannot read %zu samples from %s\n", x.size(), argv[2]);
            return 2;
        }
        std::fclose(f);
        const auto code = gnsship::glonass_l1_ca_acquisition_code(conf);
        std::vector<gnsship::Acq_Outcome> out;
        if (!acq.set_local_code(code.data()) || !acq.init_fdma(bias) || !acq.acquisition_core_fdma(x.data(), 0, out) || out.size() != bias.size()) {
            std::fprintf(stderr, "FDMA sweep failed: %s\n", acq.last_error());
            return 1;
        }
        for (const auto& o : out) print(o);
        gnsship::Acq_Outcome one;
        if (acq.set_gnss_synchro("1G", 99) || !acq.set_gnss_synchro("1G", prn) || !acq.acquisition_core(x.data(), 0, one)) {
            std::fprintf(stderr, "per-PRN acquisition failed: %s\n", acq.last_error());
            return 1;
        }
        std::printf("bias %d\n", acq.doppler_bias());
        print(one);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
