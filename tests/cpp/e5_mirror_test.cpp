// e5_mirror_test — Galileo E5a / E5b through the C++ mirror (include/gnsship_cpp.hpp).
//
//   e5_mirror_test codes OUT.bin
//       the mirror's generators under the reference's names, written as raw floats in this order: the "5X" primary
//       of PRN 11 (complex); the "7Q" primary of PRN 50 (complex); "5I" of PRN 1 sampled at 12.5 Msps with
//       chip_shift 3 (complex); "7X" of PRN 50 sampled at 10 Msps (complex).  Then, as text on stdout, the E5a-Q
//       secondary code of PRN 11 and the E5b-Q one of PRN 50.  Out-of-range PRNs and signal ids of the other band
//       must be refused.  Needs no device.  tests/test_cpp_mirror_e5.py compares everything with the C ABI's output.
//
//   e5_mirror_test 5X|7X PILOT IF.bin FS PRN ACQ_DELAY ACQ_DOPPLER ACQ_STAMP FIRST_SAMPLE EPOCHS OUT.bin
//       one channel with Dll_Pll_Conf system 'E' / signal "5X" or "7X" and track_pilot = PILOT (1 / 0), the codes from
//       the mirror's X primary as the block splits it (imaginary part tracked, real part the data code; data-only: the
//       real part tracked), Dll_Pll_Veml_Tracking_Hip::start_tracking + work over an IF file (gr_complex samples, the
//       first one absolute sample FIRST_SAMPLE).  The epoch records are written as raw gnsship_trk_epoch structs.
//       vector_length is left at 0 and extend_correlation_symbols at 0 (pilot) / 25 (data-only): the mirror applies
//       the adapters' rules.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gnsship_cpp.hpp"

static int write_codes(const char* path)
{
    std::vector<float> out;
    std::vector<std::complex<float>> z(10230);
    auto put = [&](const std::vector<std::complex<float>>& v) {
        out.insert(out.end(), reinterpret_cast<const float*>(v.data()), reinterpret_cast<const float*>(v.data()) + 2 * v.size());
    };
    const std::array<char, 3> x5 = {{'5', 'X', '\0'}}, q7 = {{'7', 'Q', '\0'}}, i5 = {{'5', 'I', '\0'}}, x7 = {{'7', 'X', '\0'}};
    if (!gnsship::galileo_e5_a_code_gen_complex_primary(z.data(), 11, x5)) return 1;
    put(z);
    if (!gnsship::galileo_e5_b_code_gen_complex_primary(z.data(), 50, q7)) return 1;
    put(z);
    z.resize(12500);
    if (gnsship::galileo_e5_a_code_gen_complex_sampled(z.data(), 1, i5, 12500000, 3) != 12500) return 1;
    put(z);
    z.resize(10000);
    if (gnsship::galileo_e5_b_code_gen_complex_sampled(z.data(), 50, x7, 10000000, 0) != 10000) return 1;
    put(z);
    z.resize(12500);
    if (gnsship::galileo_e5_a_code_gen_complex_primary(z.data(), 0, x5) || gnsship::galileo_e5_a_code_gen_complex_primary(z.data(), 51, x5) ||
        gnsship::galileo_e5_a_code_gen_complex_primary(z.data(), 1, x7) || gnsship::galileo_e5_b_code_gen_complex_primary(z.data(), 1, x5) ||
        gnsship::galileo_e5_b_code_gen_complex_sampled(z.data(), 51, x7, 12500000, 0) >= 0 || !gnsship::galileo_e5a_q_secondary_code(48).empty() ||
        !gnsship::galileo_e5b_q_secondary_code(51).empty()) {
        std::fprintf(stderr, "an out-of-range PRN or a signal id of the other band was accepted\n");
        return 1;
    }
    std::printf("%s\n%s\nout-of-range PRNs refused\n", gnsship::galileo_e5a_q_secondary_code(11).c_str(), gnsship::galileo_e5b_q_secondary_code(50).c_str());
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
    if (argc != 12 || (std::strcmp(argv[1], "5X") != 0 && std::strcmp(argv[1], "7X") != 0)) {
        std::fprintf(stderr, "usage: e5_mirror_test codes OUT.bin\n"
                             "       e5_mirror_test 5X|7X PILOT IF.bin FS PRN ACQ_DELAY ACQ_DOPPLER ACQ_STAMP FIRST_SAMPLE EPOCHS OUT.bin\n");
        return 2;
    }
    const bool band_b = argv[1][0] == '7';
    const bool pilot = std::atoi(argv[2]) != 0;
    const double fs = std::atof(argv[4]);
    const int prn = std::atoi(argv[5]);
    const double delay = std::atof(argv[6]), doppler = std::atof(argv[7]);
    const uint64_t stamp = std::strtoull(argv[8], nullptr, 10), first = std::strtoull(argv[9], nullptr, 10);
    const int epochs = std::atoi(argv[10]);
    std::FILE* f = std::fopen(argv[3], "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[3]);
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
    std::vector<std::complex<float>> aux(10230);
    const std::array<char, 3> id = {{band_b ? '7' : '5', 'X', '\0'}};
    if (!(band_b ? gnsship::galileo_e5_b_code_gen_complex_primary(aux.data(), prn, id) : gnsship::galileo_e5_a_code_gen_complex_primary(aux.data(), prn, id))) {
        std::fprintf(stderr, "no code for PRN %d\n", prn);
        return 1;
    }
    std::vector<float> i_code(10230), q_code(10230);
    for (size_t i = 0; i < aux.size(); i++) {
        i_code[i] = aux[i].real();
        q_code[i] = aux[i].imag();
    }
    gnsship::Dll_Pll_Conf conf;  // Dll_Pll_Conf defaults; slope / spc / y_intercept are derived by the engine
    conf.fs_in = fs;
    conf.vector_length = 0;  // the mirror sets round(fs / 1000)
    conf.system = 'E';
    std::snprintf(conf.signal, sizeof(conf.signal), "%s", argv[1]);
    conf.track_pilot = pilot;
    conf.extend_correlation_symbols = pilot ? 0 : 25;  // raised to 1; data-only: capped at the I secondary length (20 / 4)
    conf.pull_in_time_s = 0;
    conf.rotator = GNSSHIP_ROTATOR_AVX;
    try {
        gnsship::Dll_Pll_Veml_Tracking_Hip trk(conf, 1);
        if (!trk.start_tracking(0, pilot ? q_code.data() : i_code.data(), pilot ? i_code.data() : nullptr, 10230, delay, doppler, stamp, first, prn)) {
            std::fprintf(stderr, "start_tracking failed: %s\n", trk.last_error());
            return 1;
        }
        std::vector<gnsship_trk_epoch> rec(static_cast<size_t>(epochs));
        const int done = trk.work(x.data(), first, static_cast<int64_t>(x.size()), epochs, rec.data());
        if (done < 0) {
            std::fprintf(stderr, "work failed: %s\n", trk.last_error());
            return 1;
        }
        std::FILE* o = std::fopen(argv[11], "wb");
        if (!o || std::fwrite(rec.data(), sizeof(gnsship_trk_epoch), rec.size(), o) != rec.size() || std::fclose(o) != 0) {
            std::fprintf(stderr, "cannot write %s\n", argv[11]);
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
