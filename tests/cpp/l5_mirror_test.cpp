// l5_mirror_test — one GPS L5 channel through the C++ mirror (include/gnsship_cpp.hpp): Dll_Pll_Conf with
// system 'G' / signal "L5", the codes from the mirror's gps_l5q_code_gen_float / gps_l5i_code_gen_float,
// Dll_Pll_Veml_Tracking_Hip::start_tracking + work over an IF file.  The epoch records are written as
// raw gnsship_trk_epoch structs; tests/test_cpp_mirror_l5.py compares them with the oracle loop's.
//
//   l5_mirror_test IF.bin FS PRN ACQ_DELAY ACQ_DOPPLER ACQ_STAMP FIRST_SAMPLE EPOCHS OUT.bin
//
// IF.bin: gr_complex samples, the first one absolute sample FIRST_SAMPLE.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gnsship_cpp.hpp"

int main(int argc, char** argv)
{
    if (argc != 10) {
        std::fprintf(stderr, "usage: l5_mirror_test IF.bin FS PRN ACQ_DELAY ACQ_DOPPLER ACQ_STAMP FIRST_SAMPLE EPOCHS OUT.bin\n");
        return 2;
    }
    const double fs = std::atof(argv[2]);
    const auto prn = static_cast<uint32_t>(std::atoi(argv[3]));
    const double delay = std::atof(argv[4]), doppler = std::atof(argv[5]);
    const uint64_t stamp = std::strtoull(argv[6], nullptr, 10), first = std::strtoull(argv[7], nullptr, 10);
    const int epochs = std::atoi(argv[8]);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
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
    std::vector<float> pilot(gnsship::GPS_L5Q_CODE_LENGTH_CHIPS), data(gnsship::GPS_L5I_CODE_LENGTH_CHIPS);
    if (!gnsship::gps_l5q_code_gen_float(pilot.data(), prn) || !gnsship::gps_l5i_code_gen_float(data.data(), prn)) {
        std::fprintf(stderr, "no L5 code for PRN %u\n", prn);
        return 1;
    }
    gnsship::Dll_Pll_Conf conf;  // Dll_Pll_Conf defaults; slope / spc / y_intercept are derived by the engine
    conf.fs_in = fs;
    conf.vector_length = static_cast<uint32_t>(std::lround(fs / (gnsship::GPS_L5I_CODE_RATE_CPS / gnsship::GPS_L5I_CODE_LENGTH_CHIPS)));
    conf.system = 'G';
    std::snprintf(conf.signal, sizeof(conf.signal), "L5");
    conf.track_pilot = true;
    conf.pull_in_time_s = 0;
    conf.rotator = GNSSHIP_ROTATOR_AVX;
    try {
        gnsship::Dll_Pll_Veml_Tracking_Hip trk(conf, 1);
        if (!trk.start_tracking(0, pilot.data(), data.data(), gnsship::GPS_L5Q_CODE_LENGTH_CHIPS, delay, doppler, stamp, first, static_cast<int>(prn))) {
            std::fprintf(stderr, "start_tracking failed: %s\n", trk.last_error());
            return 1;
        }
        std::vector<gnsship_trk_epoch> rec(static_cast<size_t>(epochs));
        const int done = trk.work(x.data(), first, static_cast<int64_t>(x.size()), epochs, rec.data());
        if (done < 0) {
            std::fprintf(stderr, "work failed: %s\n", trk.last_error());
            return 1;
        }
        std::FILE* o = std::fopen(argv[9], "wb");
        if (!o || std::fwrite(rec.data(), sizeof(gnsship_trk_epoch), rec.size(), o) != rec.size() || std::fclose(o) != 0) {
            std::fprintf(stderr, "cannot write %s\n", argv[9]);
            return 2;
        }
        std::printf("l5 mirror: %d epochs, state %d, last Doppler %.3f Hz, CN0 %.2f dB-Hz\n", done, trk.state(0),
            rec[static_cast<size_t>(done > 0 ? done - 1 : 0)].carrier_doppler_hz, rec[static_cast<size_t>(done > 0 ? done - 1 : 0)].cn0_db_hz);
        // a second engine with track_pilot = false must be refused (the block's interchange_iq path)
        conf.track_pilot = false;
        try {
            gnsship::Dll_Pll_Veml_Tracking_Hip bad(conf, 1);
            std::fprintf(stderr, "track_pilot = false was accepted\n");
            return 1;
        } catch (const std::invalid_argument& e) {
            std::printf("data-only tracking refused: %s\n", e.what());
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
