// The GPS CNAV telemetry mirror (include/gnsship_cpp.hpp Gps_L2c_Telemetry_Decoder_Hip, Gps_L5_Telemetry_Decoder_Hip,
// gps_l2c_tlm_conf, gps_l5_tlm_conf).
//   cnav_mirror_test confs                    prints both configurations (no GPU)
//   cnav_mirror_test run FILE N C CUT SIGNAL  on the GPU: FILE holds N rounds × C channels of float32 CNAV symbols, SIGNAL
//                                             is l2c or l5.  One decoder takes them through work_symbols in runs of CUT
//                                             rounds; channel C-1 gets reset() after the first run.  Per message a line
//                                             "msg <channel> <symbol_counter> <prn> <msg_id> <tow> <alert> <delay> <part>
//                                             <flags> <38 bytes in hex>", per run and channel a line "fault <run>
//                                             <channel>" where one was raised and a line "stream <run> <channel> <sum of
//                                             tow_ms mod 2^32> <sum of sflags>", at the end per channel a line "state
//                                             <channel> ..." (the block's members, then per part the scalars and the sums
//                                             of the arrays).  Then the same stream goes through work_records as tracking
//                                             records (every second round an entry that is no symbol; the symbol is in the
//                                             prompt this signal reads, its negative in the other): lines "rmsg ..." as
//                                             above with the sample counter appended.  The Python test holds the
//                                             expected values.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "gnsship_cpp.hpp"

static void print_messages(const char* tag, const gnsship::Gps_Cnav_Telemetry_Decoder_Hip& d, int C, bool with_sample)
{
    const int mpr = d.messages_per_run();
    for (int c = 0; c < C; c++)
        for (int k = 0; k < d.counts()[static_cast<size_t>(c)]; k++) {
            const gnsship_cnav_message& m = d.messages()[static_cast<size_t>(c) * mpr + k];
            std::printf("%s %d %llu %u %u %u %u %u %u %u ", tag, m.channel, static_cast<unsigned long long>(m.symbol_counter), m.prn, m.msg_id, m.tow,
                m.alert, m.delay, m.part, m.flags);
            for (int b = 0; b < 38; b++) std::printf("%02x", m.raw[b]);
            if (with_sample) std::printf(" %llu", static_cast<unsigned long long>(m.sample_counter));
            std::printf("\n");
        }
}

static std::unique_ptr<gnsship::Gps_Cnav_Telemetry_Decoder_Hip> make(bool l5, int max_rounds, int C)
{
    if (l5) return std::make_unique<gnsship::Gps_L5_Telemetry_Decoder_Hip>(gnsship::gps_l5_tlm_conf(max_rounds), C);
    return std::make_unique<gnsship::Gps_L2c_Telemetry_Decoder_Hip>(gnsship::gps_l2c_tlm_conf(max_rounds), C);
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "confs") == 0) {
        const gnsship_cnav_conf a = gnsship::gps_l2c_tlm_conf(600), b = gnsship::gps_l5_tlm_conf(1200);
        std::printf("l2c max_rounds %d signal %d reserved %d messages_per_run %d size %zu state %zu\n", a.max_rounds, a.signal, a.reserved,
            GNSSHIP_CNAV_MESSAGES_PER_RUN(a.max_rounds), sizeof(gnsship_cnav_message), sizeof(gnsship_cnav_state));
        std::printf("l5 max_rounds %d signal %d reserved %d messages_per_run %d size %zu state %zu\n", b.max_rounds, b.signal, b.reserved,
            GNSSHIP_CNAV_MESSAGES_PER_RUN(b.max_rounds), sizeof(gnsship_cnav_message), sizeof(gnsship_cnav_state));
        return 0;
    }
    if (argc != 7 || std::strcmp(argv[1], "run") != 0) {
        std::fprintf(stderr, "usage: cnav_mirror_test confs | run FILE N C CUT l2c|l5\n");
        return 2;
    }
    const int n = std::atoi(argv[3]), C = std::atoi(argv[4]), cut = std::atoi(argv[5]);
    const bool l5 = std::strcmp(argv[6], "l5") == 0;
    if (n < 1 || n > 100000 || C < 2 || C > 64 || cut < 1 || (!l5 && std::strcmp(argv[6], "l2c") != 0)) return 2;
    std::vector<float> sym(static_cast<size_t>(n) * C);
    std::FILE* fp = std::fopen(argv[2], "rb");
    if (!fp || std::fread(sym.data(), sizeof(float), sym.size(), fp) != sym.size()) {
        std::fprintf(stderr, "cannot read %zu floats from %s\n", sym.size(), argv[2]);
        return 2;
    }
    std::fclose(fp);
    try {
        auto dec = make(l5, cut, C);
        int run = 0;
        for (int r = 0; r < n; r += cut, run++) {
            const int m = n - r < cut ? n - r : cut;
            if (!dec->work_symbols(sym.data() + static_cast<size_t>(r) * C, nullptr, nullptr, m)) {
                std::printf("work_symbols failed: %s\n", dec->last_error().c_str());
                return 1;
            }
            print_messages("msg", *dec, C, false);
            for (int c = 0; c < C; c++) {
                if (dec->faults()[static_cast<size_t>(c)]) std::printf("fault %d %d\n", run, c);
                uint32_t tow = 0, sf = 0;
                for (int k = 0; k < dec->rounds(); k++) {
                    tow += dec->tow_ms()[static_cast<size_t>(k) * C + c];
                    sf += dec->sflags()[static_cast<size_t>(k) * C + c];
                }
                std::printf("stream %d %d %u %u\n", run, c, tow, sf);
            }
            if (run == 0 && !dec->reset(C - 1)) return 1;
        }
        for (int c = 0; c < C; c++) {
            const gnsship_cnav_state s = dec->state(c);
            std::printf("state %d %llu %llu %.17g %u %u %d %d %d", c, static_cast<unsigned long long>(s.symbol_counter),
                static_cast<unsigned long long>(s.last_valid_preamble), s.tow_s, s.tow_ms, s.tow_at_preamble, s.pll_180, s.valid_word, s.sent_tlm_failed);
            for (int k = 0; k < 2; k++) {
                const gnsship_cnav_part& p = s.part[k];
                uint64_t metrics = 0, decisions = 0, symbols = 0, decoded = 0;
                for (int i = 0; i < 64; i++) {
                    metrics += static_cast<uint64_t>(p.metrics[0][i]) * (i + 1) + static_cast<uint64_t>(p.metrics[1][i]) * (i + 65);
                    decisions += static_cast<uint64_t>(p.decisions[i][0]) * (2 * i + 1) + static_cast<uint64_t>(p.decisions[i][1]) * (2 * i + 2);
                    decoded += static_cast<uint64_t>(p.decoded[i]) * (i + 1);
                }
                for (int i = 0; i < 128; i++) symbols += static_cast<uint64_t>(p.symbols[i]) * (i + 1);
                std::printf(" %u %u %u %u %d %d %d %d %d %d %llu %llu %llu %llu", p.n_symbols, p.n_decoded, p.n_crc_fail, p.decisions_index,
                    p.old_is_metrics2, p.preamble_seen, p.invert, p.message_lock, p.crc_ok, p.init, static_cast<unsigned long long>(metrics),
                    static_cast<unsigned long long>(decisions), static_cast<unsigned long long>(symbols), static_cast<unsigned long long>(decoded));
            }
            std::printf("\n");
        }
        std::printf("too_many %s\n", dec->work_symbols(sym.data(), nullptr, nullptr, cut + 1) ? "accepted" : "refused");
        std::printf("bad_channel %s\n", dec->reset(C) || dec->new_channel(-1) || dec->set_state(C, dec->state(0)) ? "accepted" : "refused");
        bool wrong_signal = false;
        try {
            gnsship::Gps_L5_Telemetry_Decoder_Hip wrong(gnsship::gps_l2c_tlm_conf(10), 1);
        } catch (const std::invalid_argument&) {
            wrong_signal = true;
        }
        std::printf("wrong_signal %s\n", wrong_signal ? "refused" : "accepted");

        // the same stream as tracking records: round 2r carries the symbol, round 2r + 1 an epoch that is no symbol
        auto rdec = make(l5, 2 * n, C);
        std::vector<gnsship_trk_epoch> rec(static_cast<size_t>(2 * n) * C);
        std::memset(rec.data(), 0, rec.size() * sizeof(gnsship_trk_epoch));
        for (int r = 0; r < n; r++)
            for (int c = 0; c < C; c++) {
                gnsship_trk_epoch& e = rec[static_cast<size_t>(2 * r) * C + c];
                const double s = sym[static_cast<size_t>(r) * C + c];
                (l5 ? e.prompt_q : e.prompt_i) = s;
                (l5 ? e.prompt_i : e.prompt_q) = -s;
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
        print_messages("rmsg", *rdec, C, true);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("cnav_mirror_test done\n");
    return 0;
}
