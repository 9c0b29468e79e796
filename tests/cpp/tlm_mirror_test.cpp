// The telemetry mirror (include/gnsship_cpp.hpp Galileo_Telemetry_Decoder_Hip, galileo_*_tlm_conf).
//   tlm_mirror_test confs                 prints the three configurations (no GPU)
//   tlm_mirror_test run FILE N C CUT      on the GPU: FILE holds N rounds × C channels of float32 I/NAV symbols.  One
//                                         Galileo_Telemetry_Decoder_Hip takes them through work_symbols in runs of CUT
//                                         rounds; channel 1 gets set_satellite() and channel C-1 reset() after the first
//                                         run.  Per emitted part a line "page <channel> <symbol_counter> <flags>
//                                         <crc_error_counter> <bits>", per run and channel a line "fault <run> <channel>"
//                                         where one was raised, at the end per channel a line "state <channel> ...".
//                                         Then the same stream goes through work_records as tracking records (every
//                                         second round an entry that is no symbol): lines "rpage ..." as above with the
//                                         sample counter appended.  The Python test holds the expected values.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gnsship_cpp.hpp"

static void print_conf(const char* name, const gnsship_tlm_conf& c)
{
    std::printf("%s frame_type %d vit_mode %d max_rounds %d reserved %d\n", name, c.frame_type, c.vit_mode, c.max_rounds, c.reserved);
}

static std::string bit_string(const uint8_t* b, size_t n)
{
    std::string s(n, '0');
    for (size_t i = 0; i < n; i++) s[i] = b[i] ? '1' : '0';
    return s;
}

static void print_pages(const char* tag, const gnsship::Galileo_Telemetry_Decoder_Hip& d, int C, bool with_sample)
{
    const int LL = d.data_length(), ppr = d.pages_per_run();
    for (int c = 0; c < C; c++)
        for (int k = 0; k < d.counts()[static_cast<size_t>(c)]; k++) {
            const size_t slot = static_cast<size_t>(c) * ppr + k;
            const gnsship_tlm_page& p = d.pages()[slot];
            std::printf("%s %d %llu %d %d %s", tag, p.channel, static_cast<unsigned long long>(p.symbol_counter), p.flags, p.crc_error_counter,
                bit_string(d.bits().data() + slot * LL, static_cast<size_t>(LL)).c_str());
            if (with_sample) std::printf(" %llu", static_cast<unsigned long long>(p.sample_counter));
            std::printf("\n");
        }
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "confs") == 0) {
        print_conf("inav", gnsship::galileo_inav_tlm_conf(600));
        print_conf("fnav", gnsship::galileo_fnav_tlm_conf(1200));
        print_conf("cnav", gnsship::galileo_cnav_tlm_conf(2500, GNSSHIP_VIT_MODE_FULL));
        return 0;
    }
    if (argc != 6 || std::strcmp(argv[1], "run") != 0) {
        std::fprintf(stderr, "usage: tlm_mirror_test confs | run FILE N C CUT\n");
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
        gnsship::Galileo_Telemetry_Decoder_Hip dec(gnsship::galileo_inav_tlm_conf(cut), C);
        int run = 0;
        for (int r = 0; r < n; r += cut, run++) {
            const int m = n - r < cut ? n - r : cut;
            if (!dec.work_symbols(sym.data() + static_cast<size_t>(r) * C, nullptr, m)) {
                std::printf("work_symbols failed: %s\n", dec.last_error().c_str());
                return 1;
            }
            print_pages("page", dec, C, false);
            for (int c = 0; c < C; c++)
                if (dec.faults()[static_cast<size_t>(c)]) std::printf("fault %d %d\n", run, c);
            if (run == 0 && (!dec.set_satellite(1) || !dec.reset(C - 1))) return 1;
        }
        for (int c = 0; c < C; c++) {
            const gnsship_tlm_state s = dec.state(c);
            std::printf("state %d %llu %llu %llu %d %d %d %d %d %d %d %d\n", c, static_cast<unsigned long long>(s.symbol_counter),
                static_cast<unsigned long long>(s.preamble_index), static_cast<unsigned long long>(s.last_valid_preamble), s.stat, s.crc_error_counter,
                s.history_size, s.pll_180, s.frame_sync, s.even_word_arrived, s.flag_crc_test, s.sent_tlm_failed);
        }
        std::printf("too_many %s\n", dec.work_symbols(sym.data(), nullptr, cut + 1) ? "accepted" : "refused");
        std::printf("bad_channel %s\n", dec.reset(C) || dec.set_satellite(-1) || dec.new_channel(C) ? "accepted" : "refused");

        // the same stream as tracking records: round 2r carries the symbol, round 2r + 1 an epoch that is no symbol
        gnsship::Galileo_Telemetry_Decoder_Hip rdec(gnsship::galileo_inav_tlm_conf(2 * n), C);
        std::vector<gnsship_trk_epoch> rec(static_cast<size_t>(2 * n) * C);
        std::memset(rec.data(), 0, rec.size() * sizeof(gnsship_trk_epoch));
        for (int r = 0; r < n; r++)
            for (int c = 0; c < C; c++) {
                gnsship_trk_epoch& e = rec[static_cast<size_t>(2 * r) * C + c];
                e.prompt_i = sym[static_cast<size_t>(r) * C + c];
                e.flags = 9;
                e.sample_counter = 1000000ull + 16000ull * static_cast<uint64_t>(r) + static_cast<uint64_t>(c);
                gnsship_trk_epoch& skip = rec[static_cast<size_t>(2 * r + 1) * C + c];
                skip.prompt_i = -e.prompt_i;
                skip.flags = 8;
            }
        if (!rdec.work_records(rec.data(), 2 * n)) {
            std::printf("work_records failed: %s\n", rdec.last_error().c_str());
            return 1;
        }
        print_pages("rpage", rdec, C, true);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("tlm_mirror_test done\n");
    return 0;
}
