// b3i_l2c_mirror_test — BeiDou B3I and GPS L2C through the C++ mirror (include/gnsship_cpp.hpp).
//
//   b3i_l2c_mirror_test codes OUT.bin
//       the mirror's generators under the reference's names, written as raw floats in this order: B3I PRN 9;
//       B3I PRN 30 with chip_shift 37; L2 CM PRN 9; B3I PRN 9 sampled at 12.5 Msps with chip_shift 37 (complex);
//       L2 CM PRN 30 sampled at 2 Msps (complex).  Out-of-range PRNs must be refused.  Needs no device.
//       tests/test_codes_b3i_l2c.py compares the file with the C ABI's output.
//
//   b3i_l2c_mirror_test B3|2S IF.bin FS PRN ACQ_DELAY ACQ_DOPPLER ACQ_STAMP FIRST_SAMPLE EPOCHS OUT.bin
//       one channel with Dll_Pll_Conf system 'C' / signal "B3" or system 'G' / signal "2S", the code from the
//       mirror's generator, Dll_Pll_Veml_Tracking_Hip::start_tracking + work over an IF file (gr_complex samples,
//       the first one absolute sample FIRST_SAMPLE).  The epoch records are written as raw gnsship_trk_epoch
//       structs; tests/test_cpp_mirror_b3i_l2c.py compares them with the oracle loop's.  vector_length,
//       extend_correlation_symbols and track_pilot are left at values the adapters would correct: the mirror applies
//       the adapters' rules.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gnsship_cpp.hpp"

static int write_codes(const char* path)
{
    std::vector<float> out;
    std::vector<float> chips(10230);
    std::vector<std::complex<float>> sampled;
    auto put = [&](const float* p, size_t n) { out.insert(out.end(), p, p + n); };
    if (!gnsship::beidou_b3i_code_gen_float(chips.data(), 9, 0)) return 1;
    put(chips.data(), chips.size());
    if (!gnsship::beidou_b3i_code_gen_float(chips.data(), 30, 37)) return 1;
    put(chips.data(), chips.size());
    if (!gnsship::gps_l2c_m_code_gen_float(chips.data(), 9)) return 1;
    put(chips.data(), chips.size());
    sampled.resize(12500);
    if (gnsship::beidou_b3i_code_gen_complex_sampled(sampled.data(), 9, 12500000, 37) != 12500) return 1;
    put(reinterpret_cast<const float*>(sampled.data()), 2 * sampled.size());
    sampled.resize(40000);
    if (gnsship::gps_l2c_m_code_gen_complex_sampled(sampled.data(), 30, 2000000) != 40000) return 1;
    put(reinterpret_cast<const float*>(sampled.data()), 2 * sampled.size());
    if (gnsship::beidou_b3i_code_gen_float(chips.data(), 0, 0) || gnsship::beidou_b3i_code_gen_float(chips.data(), 64, 0) ||
        gnsship::gps_l2c_m_code_gen_float(chips.data(), 0) || gnsship::gps_l2c_m_code_gen_float(chips.data(), 51) ||
        gnsship::beidou_b3i_code_gen_complex_sampled(sampled.data(), 64, 12500000, 0) >= 0 ||
        gnsship::gps_l2c_m_code_gen_complex_sampled(sampled.data(), 51, 2000000) >= 0) {
        std::fprintf(stderr, "an out-of-range PRN was accepted\n");
        return 1;
    }
    std::printf("out-of-range PRNs refused\n");
    std::FILE* o = std::fopen(path, "wb");
    if (!o || std::fwrite(out.data(), sizeof(float), out.size(), o) != out.size() || std::fclose(o) != 0) {
        std::fprintf(stderr, "cannot write %s\n", path);
        return 2;
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && std::strcmp(argv[1], "codes") == 0) return write_codes(argv[2]);
    if (argc != 11 || (std::strcmp(argv[1], "B3") != 0 && std::strcmp(argv[1], "2S") != 0)) {
        std::fprintf(stderr, "usage: b3i_l2c_mirror_test codes OUT.bin\n"
                             "       b3i_l2c_mirror_test B3|2S IF.bin FS PRN ACQ_DELAY ACQ_DOPPLER ACQ_STAMP FIRST_SAMPLE EPOCHS OUT.bin\n");
        return 2;
    }
    const bool l2c = std::strcmp(argv[1], "2S") == 0;
    const double fs = std::atof(argv[3]);
    const auto prn = static_cast<uint32_t>(std::atoi(argv[4]));
    const double delay = std::atof(argv[5]), doppler = std::atof(argv[6]);
    const uint64_t stamp = std::strtoull(argv[7], nullptr, 10), first = std::strtoull(argv[8], nullptr, 10);
    const int epochs = std::atoi(argv[9]);
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[2]);
        return 2;
    }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<std::complex<float>> x(static_cast<size_t>(bytes) / sizeof(std::complex<float>));
    const size_t got = std::fread(x.data(), sizeof(std::complex<float>), x.size(), f);
    std::fclose(f);
    if (got != x.size() || x.empty() || epochs < 1) {
        std::fprintf(stderr, "short read / empty input\n");
        return 2;
    }
    std::vector<float> code(10230);
    if (!(l2c ? gnsship::gps_l2c_m_code_gen_float(code.data(), prn) : gnsship::beidou_b3i_code_gen_float(code.data(), static_cast<int32_t>(prn), 0))) {
        std::fprintf(stderr, "no code for PRN %u\n", prn);
        return 1;
    }
    gnsship::Dll_Pll_Conf conf;  // Dll_Pll_Conf defaults; slope / spc / y_intercept are derived by the engine
    conf.fs_in = fs;
    conf.vector_length = 0;  // the mirror sets round(fs / 1000) or round(fs / 50)
    conf.system = l2c ? 'G' : 'C';
    std::snprintf(conf.signal, sizeof(conf.signal), "%s", l2c ? "2S" : "B3");
    conf.track_pilot = true;                        // forced to false for both signals
    conf.extend_correlation_symbols = l2c ? 4 : 0;  // L2C: forced to 1; B3I: raised to 1
    if (l2c) {                                      // the reference's L2C loop bandwidths
        conf.pll_bw_hz = 2.0F;
        conf.dll_bw_hz = 0.25F;
    }
    conf.pull_in_time_s = 0;
    conf.rotator = GNSSHIP_ROTATOR_AVX;
    try {
        gnsship::Dll_Pll_Veml_Tracking_Hip trk(conf, 1);
        if (!trk.start_tracking(0, code.data(), nullptr, 10230, delay, doppler, stamp, first, static_cast<int>(prn))) {
            std::fprintf(stderr, "start_tracking failed: %s\n", trk.last_error());
            return 1;
        }
        std::vector<gnsship_trk_epoch> rec(static_cast<size_t>(epochs));
        const int done = trk.work(x.data(), first, static_cast<int64_t>(x.size()), epochs, rec.data());
        if (done < 0) {
            std::fprintf(stderr, "work failed: %s\n", trk.last_error());
            return 1;
        }
        std::FILE* o = std::fopen(argv[10], "wb");
        if (!o || std::fwrite(rec.data(), sizeof(gnsship_trk_epoch), rec.size(), o) != rec.size() || std::fclose(o) != 0) {
            std::fprintf(stderr, "cannot write %s\n", argv[10]);
            return 2;
        }
        std::printf("%s mirror: %d epochs, state %d, last Doppler %.3f Hz, CN0 %.2f dB-Hz\n", argv[1], done, trk.state(0),
            rec[static_cast<size_t>(done > 0 ? done - 1 : 0)].carrier_doppler_hz, rec[static_cast<size_t>(done > 0 ? done - 1 : 0)].cn0_db_hz);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
