// The BeiDou D1/D2 telemetry mirror (include/gnsship_cpp.hpp Beidou_B1i_Telemetry_Decoder_Hip,
// Beidou_B3i_Telemetry_Decoder_Hip, beidou_b1i_tlm_conf, beidou_b3i_tlm_conf).
//   dnav_mirror_test confs                    prints both configurations (no GPU)
//   dnav_mirror_test run FILE N C CUT SIGNAL PRN...
//                                             on the GPU: FILE holds N rounds × C channels of float32 symbols, SIGNAL is
//                                             b1i or b3i, and there are C PRNs.  One decoder, channel c a new object on
//                                             PRN c, takes them through work_symbols in runs of CUT rounds; channel C-1
//                                             gets reset() after the first run and channel 0 set_satellite(3) and back to
//                                             its own PRN around the second.  Per subframe a line "sub <channel>
//                                             <symbol_counter> <fra_id> <pnum> <sow> <corrected_mask> <tow> <flags> <ten words
//                                             in hex>", per run and channel a line "stream <run> <channel> <sum of tow_ms mod
//                                             2^32> <sum of sflags>", at the end per channel a line "state <channel> ..."
//                                             with the members in the order of gnsship_dnav_state.  Then the same stream
//                                             goes through work_records as tracking records (every second round an entry
//                                             that is no symbol): lines "rsub ..." as above with the sample counter
//                                             appended.  The Python test holds the expected values.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "gnsship_cpp.hpp"

static void print_subframes(const char* tag, const gnsship::Beidou_Dnav_Telemetry_Decoder_Hip& d, int C, bool with_sample)
{
    const int spr = d.subframes_per_run();
    for (int c = 0; c < C; c++)
        for (int k = 0; k < d.counts()[static_cast<size_t>(c)]; k++) {
            const gnsship_dnav_subframe& s = d.subframes()[static_cast<size_t>(c) * spr + k];
            std::printf("%s %d %llu %d %d %u %u %u %u", tag, s.channel, static_cast<unsigned long long>(s.symbol_counter), s.fra_id, s.pnum, s.sow,
                s.corrected_mask, s.tow_at_current_symbol_ms, s.flags);
            for (int w = 0; w < 10; w++) std::printf(" %08x", s.words[w]);
            if (with_sample) std::printf(" %llu", static_cast<unsigned long long>(s.sample_counter));
            std::printf("\n");
        }
}

static std::unique_ptr<gnsship::Beidou_Dnav_Telemetry_Decoder_Hip> make(bool b3i, int max_rounds, int C, const std::vector<int>& prns)
{
    std::unique_ptr<gnsship::Beidou_Dnav_Telemetry_Decoder_Hip> d;
    if (b3i) d = std::make_unique<gnsship::Beidou_B3i_Telemetry_Decoder_Hip>(gnsship::beidou_b3i_tlm_conf(max_rounds), C);
    else d = std::make_unique<gnsship::Beidou_B1i_Telemetry_Decoder_Hip>(gnsship::beidou_b1i_tlm_conf(max_rounds), C);
    for (int c = 0; c < C; c++)
        if (!d->new_channel(c, prns[static_cast<size_t>(c)])) throw std::runtime_error("new_channel: " + d->last_error());
    return d;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "confs") == 0) {
        const gnsship_dnav_conf a = gnsship::beidou_b1i_tlm_conf(601), b = gnsship::beidou_b3i_tlm_conf(1300);
        std::printf("b1i max_rounds %d signal %d reserved %d subframes_per_run %d size %zu state %zu\n", a.max_rounds, a.signal, a.reserved,
            GNSSHIP_DNAV_SUBFRAMES_PER_RUN(a.max_rounds), sizeof(gnsship_dnav_subframe), sizeof(gnsship_dnav_state));
        std::printf("b3i max_rounds %d signal %d reserved %d subframes_per_run %d size %zu state %zu\n", b.max_rounds, b.signal, b.reserved,
            GNSSHIP_DNAV_SUBFRAMES_PER_RUN(b.max_rounds), sizeof(gnsship_dnav_subframe), sizeof(gnsship_dnav_state));
        return 0;
    }
    if (argc < 8 || std::strcmp(argv[1], "run") != 0) {
        std::fprintf(stderr, "usage: dnav_mirror_test confs | run FILE N C CUT b1i|b3i PRN...\n");
        return 2;
    }
    const int n = std::atoi(argv[3]), C = std::atoi(argv[4]), cut = std::atoi(argv[5]);
    const bool b3i = std::strcmp(argv[6], "b3i") == 0;
    if (n < 1 || n > 100000 || C < 2 || C > 64 || cut < 1 || argc != 7 + C || (!b3i && std::strcmp(argv[6], "b1i") != 0)) return 2;
    std::vector<int> prns;
    for (int c = 0; c < C; c++) prns.push_back(std::atoi(argv[7 + c]));
    std::vector<float> sym(static_cast<size_t>(n) * C);
    std::FILE* fp = std::fopen(argv[2], "rb");
    if (!fp || std::fread(sym.data(), sizeof(float), sym.size(), fp) != sym.size()) {
        std::fprintf(stderr, "cannot read %zu floats from %s\n", sym.size(), argv[2]);
        return 2;
    }
    std::fclose(fp);
    try {
        auto dec = make(b3i, cut, C, prns);
        int run = 0;
        for (int r = 0; r < n; r += cut, run++) {
            const int m = n - r < cut ? n - r : cut;
            if (run == 1 && !dec->set_satellite(0, 3)) return 1;
            if (!dec->work_symbols(sym.data() + static_cast<size_t>(r) * C, nullptr, nullptr, m)) {
                std::printf("work_symbols failed: %s\n", dec->last_error().c_str());
                return 1;
            }
            print_subframes("sub", *dec, C, false);
            for (int c = 0; c < C; c++) {
                uint32_t tow = 0, sf = 0;
                for (int k = 0; k < dec->rounds(); k++) {
                    tow += dec->tow_ms()[static_cast<size_t>(k) * C + c];
                    sf += dec->sflags()[static_cast<size_t>(k) * C + c];
                }
                std::printf("stream %d %d %u %u\n", run, c, tow, sf);
            }
            if (run == 0 && !dec->reset(C - 1)) return 1;
            if (run == 1 && !dec->set_satellite(0, prns[0])) return 1;
        }
        for (int c = 0; c < C; c++) {
            const gnsship_dnav_state s = dec->state(c);
            std::printf("state %d %llu %llu %llu %u %u %u %u %d %d %d %d %d %d %d %d %d %d %d\n", c, static_cast<unsigned long long>(s.symbol_counter),
                static_cast<unsigned long long>(s.preamble_index), static_cast<unsigned long long>(s.last_valid_preamble), s.tow_at_preamble_ms,
                s.tow_at_current_symbol_ms, s.sow, s.symbol_duration_ms, s.stat, s.crc_error_counter, s.history_size, s.prn, s.sow_set, s.frame_sync,
                s.valid_word, s.new_sow_available, s.sent_tlm_failed, s.d2_decoder, s.d2_timing);
        }
        std::printf("too_many %s\n", dec->work_symbols(sym.data(), nullptr, nullptr, cut + 1) ? "accepted" : "refused");
        std::printf("bad_channel %s\n", dec->reset(C) || dec->new_channel(-1, 3) || dec->set_satellite(C, 3) ? "accepted" : "refused");
        std::printf("bad_prn %s\n", dec->set_satellite(0, 64) || dec->new_channel(0, -1) ? "accepted" : "refused");
        bool wrong_signal = false;
        try {
            gnsship::Beidou_B3i_Telemetry_Decoder_Hip wrong(gnsship::beidou_b1i_tlm_conf(10), 1);
        } catch (const std::invalid_argument&) {
            wrong_signal = true;
        }
        std::printf("wrong_signal %s\n", wrong_signal ? "refused" : "accepted");

        // the same stream as tracking records: round 2r carries the symbol, round 2r + 1 an epoch that is no symbol
        auto rdec = make(b3i, 2 * n, C, prns);
        std::vector<gnsship_trk_epoch> rec(static_cast<size_t>(2 * n) * C);
        std::memset(rec.data(), 0, rec.size() * sizeof(gnsship_trk_epoch));
        for (int r = 0; r < n; r++)
            for (int c = 0; c < C; c++) {
                gnsship_trk_epoch& e = rec[static_cast<size_t>(2 * r) * C + c];
                const double s = sym[static_cast<size_t>(r) * C + c];
                e.prompt_i = s;
                e.prompt_q = -s;
                e.flags = 9;
                e.sample_counter = 1000000ull + 16000ull * static_cast<uint64_t>(r) + static_cast<uint64_t>(c);
                gnsship_trk_epoch& skip = rec[static_cast<size_t>(2 * r + 1) * C + c];
                skip.prompt_i = skip.prompt_q = -s;
                skip.flags = 8;
            }
        if (!rdec->work_records(rec.data(), 2 * n)) {
            std::printf("work_records failed: %s\n", rdec->last_error().c_str());
            return 1;
        }
        print_subframes("rsub", *rdec, C, true);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("dnav_mirror_test done\n");
    return 0;
}
