// The GPS L1 C/A telemetry mirror (include/gnsship_cpp.hpp Gps_L1_Ca_Telemetry_Decoder_Hip, gps_l1_ca_tlm_conf).
//   lnav_mirror_test confs                prints the configuration (no GPU)
//   lnav_mirror_test run FILE N C CUT     on the GPU: FILE holds N rounds × C channels of float32 LNAV symbols.  One
//                                         Gps_L1_Ca_Telemetry_Decoder_Hip takes them through work_symbols in runs of CUT
//                                         rounds; channel 1 gets set_satellite() and channel C-1 reset() after the first
//                                         run.  Per emitted subframe a line "sub <channel> <symbol_counter> <id> <tow_s>
//                                         <crc_error_counter> <parity_fail_mask> <flags> <ten words in hex>", per run and
//                                         channel a line "fault <run> <channel>" where one was raised and a line
//                                         "stream <run> <channel> <sum of tow_ms mod 2^32> <sum of sflags>", at the end
//                                         per channel a line "state <channel> ...".  Then the same stream goes through
//                                         work_records as tracking records (every second round an entry that is no
//                                         symbol, channel 1 with the 180° flag): lines "rsub ..." as above with the
//                                         sample counter appended.  The Python test holds the expected values.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gnsship_cpp.hpp"

static void print_subframes(const char* tag, const gnsship::Gps_L1_Ca_Telemetry_Decoder_Hip& d, int C, bool with_sample)
{
    const int spr = d.subframes_per_run();
    for (int c = 0; c < C; c++)
        for (int k = 0; k < d.counts()[static_cast<size_t>(c)]; k++) {
            const gnsship_lnav_subframe& s = d.subframes()[static_cast<size_t>(c) * spr + k];
            std::printf("%s %d %llu %d %u %d %u %d", tag, s.channel, static_cast<unsigned long long>(s.symbol_counter), s.subframe_id, s.tow_s,
                s.crc_error_counter, s.parity_fail_mask, s.flags);
            for (int w = 0; w < 10; w++) std::printf(" %08x", s.words[w]);
            if (with_sample) std::printf(" %llu", static_cast<unsigned long long>(s.sample_counter));
            std::printf("\n");
        }
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "confs") == 0) {
        const gnsship_lnav_conf c = gnsship::gps_l1_ca_tlm_conf(600);
        std::printf("lnav max_rounds %d reserved %d subframes_per_run %d size %zu\n", c.max_rounds, c.reserved,
            GNSSHIP_LNAV_SUBFRAMES_PER_RUN(c.max_rounds), sizeof(gnsship_lnav_subframe));
        return 0;
    }
    if (argc != 6 || std::strcmp(argv[1], "run") != 0) {
        std::fprintf(stderr, "usage: lnav_mirror_test confs | run FILE N C CUT\n");
        return 2;
    }
    const int n = std::atoi(argv[3]), C = std::atoi(argv[4]), cut = std::atoi(argv[5]);
    if (n < 1 || n > 100000 || C < 2 || C > 64 || cut < 1) return 2;
    std::vector<float> sym(static_cast<size_t>(n) * C);
    std::FILE* fp = std::fopen(argv[2], "rb");
    if (!fp || std::fread(sym.data(), sizeof(float), sym.size(), fp) != sym.size()) {
        std::fprintf(stderr, "cannot read %zu floats from %s\n", sym.size(), argv[2]);
        return 2;
    }
    std::fclose(fp);
    try {
        gnsship::Gps_L1_Ca_Telemetry_Decoder_Hip dec(gnsship::gps_l1_ca_tlm_conf(cut), C);
        int run = 0;
        for (int r = 0; r < n; r += cut, run++) {
            const int m = n - r < cut ? n - r : cut;
            if (!dec.work_symbols(sym.data() + static_cast<size_t>(r) * C, nullptr, nullptr, m)) {
                std::printf("work_symbols failed: %s\n", dec.last_error().c_str());
                return 1;
            }
            print_subframes("sub", dec, C, false);
            for (int c = 0; c < C; c++) {
                if (dec.faults()[static_cast<size_t>(c)]) std::printf("fault %d %d\n", run, c);
                uint32_t tow = 0, sf = 0;
                for (int k = 0; k < dec.rounds(); k++) {
                    tow += dec.tow_ms()[static_cast<size_t>(k) * C + c];
                    sf += dec.sflags()[static_cast<size_t>(k) * C + c];
                }
                std::printf("stream %d %d %u %u\n", run, c, tow, sf);
            }
            if (run == 0 && (!dec.set_satellite(1) || !dec.reset(C - 1))) return 1;
        }
        for (int c = 0; c < C; c++) {
            const gnsship_lnav_state s = dec.state(c);
            std::printf("state %d %llu %llu %llu %llu %u %u %u %u %d %d %d %d %d %d %d\n", c, static_cast<unsigned long long>(s.symbol_counter),
                static_cast<unsigned long long>(s.preamble_index), static_cast<unsigned long long>(s.last_valid_preamble),
                static_cast<unsigned long long>(s.subframes_tried), s.prev_word, s.tow_at_preamble_ms, s.tow_at_current_symbol_ms, s.nav_tow_s, s.stat,
                s.crc_error_counter, s.history_size, s.pll_180, s.frame_sync, s.tow_set, s.sent_tlm_failed);
        }
        std::printf("too_many %s\n", dec.work_symbols(sym.data(), nullptr, nullptr, cut + 1) ? "accepted" : "refused");
        std::printf("bad_channel %s\n", dec.reset(C) || dec.set_satellite(-1) || dec.new_channel(C) ? "accepted" : "refused");

        // the same stream as tracking records: round 2r carries the symbol, round 2r + 1 an epoch that is no symbol
        gnsship::Gps_L1_Ca_Telemetry_Decoder_Hip rdec(gnsship::gps_l1_ca_tlm_conf(2 * n), C);
        std::vector<gnsship_trk_epoch> rec(static_cast<size_t>(2 * n) * C);
        std::memset(rec.data(), 0, rec.size() * sizeof(gnsship_trk_epoch));
        for (int r = 0; r < n; r++)
            for (int c = 0; c < C; c++) {
                gnsship_trk_epoch& e = rec[static_cast<size_t>(2 * r) * C + c];
                e.prompt_i = sym[static_cast<size_t>(r) * C + c];
                e.flags = 9 | (c == 1 ? 4 : 0);
                e.sample_counter = 1000000ull + 16000ull * static_cast<uint64_t>(r) + static_cast<uint64_t>(c);
                gnsship_trk_epoch& skip = rec[static_cast<size_t>(2 * r + 1) * C + c];
                skip.prompt_i = -e.prompt_i;
                skip.flags = 8;
            }
        if (!rdec.work_records(rec.data(), 2 * n)) {
            std::printf("work_records failed: %s\n", rdec.last_error().c_str());
            return 1;
        }
        print_subframes("rsub", rdec, C, true);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("lnav_mirror_test done\n");
    return 0;
}
