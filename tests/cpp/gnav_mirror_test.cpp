// The GLONASS GNAV telemetry mirror (include/gnsship_cpp.hpp Glonass_L1_Ca_Telemetry_Decoder_Hip,
// Glonass_L2_Ca_Telemetry_Decoder_Hip, glonass_l1_ca_tlm_conf, glonass_l2_ca_tlm_conf).
//   gnav_mirror_test confs                    prints both configurations (no GPU)
//   gnav_mirror_test run FILE N C CUT SIGNAL PRN...
//                                             on the GPU: FILE holds N rounds × C channels of float32 symbols, SIGNAL is
//                                             l1 or l2, and there are C PRNs.  One decoder, channel c a new object on PRN
//                                             c, takes them through work_symbols in runs of CUT rounds; channel 0 gets
//                                             set_satellite(9) before the second run.  Per string a line "str <channel>
//                                             <symbol_counter> <prn> <string_id> <flipped_bit> <tow_ms> <flags> <d_TOW bits in
//                                             hex> <three words in hex>", per run and channel a line "stream <run> <channel>
//                                             <sum of tow_ms mod 2^32> <sum of sflags>", at the end per channel a line
//                                             "state <channel> ..." with the scalar members in the order of
//                                             gnsship_gnav_state (doubles as their bits) and the sums of the three arrays.
//                                             Then channel 1's state is set on channel 0 ("copy" line: the state read back),
//                                             and the same stream goes through work_records as tracking records (every second
//                                             round an entry that is no symbol): lines "rstr ..." as above with the sample
//                                             counter appended.  The Python test holds the expected values.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "gnsship_cpp.hpp"

static unsigned long long bits_of(double v)
{
    unsigned long long u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

static void print_strings(const char* tag, const gnsship::Glonass_Gnav_Telemetry_Decoder_Hip& d, int C, bool with_sample)
{
    const int spr = d.strings_per_run();
    for (int c = 0; c < C; c++)
        for (int k = 0; k < d.counts()[static_cast<size_t>(c)]; k++) {
            const gnsship_gnav_string& s = d.strings()[static_cast<size_t>(c) * spr + k];
            std::printf("%s %d %llu %d %d %d %u %u %016llx %08x %08x %08x", tag, s.channel, static_cast<unsigned long long>(s.symbol_counter), s.prn,
                s.string_id, s.flipped_bit, s.tow_at_current_symbol_ms, s.flags, bits_of(s.tow), s.bits[0], s.bits[1], s.bits[2]);
            if (with_sample) std::printf(" %llu", static_cast<unsigned long long>(s.sample_counter));
            std::printf("\n");
        }
}

static void print_state(const char* tag, int c, const gnsship_gnav_state& s)
{
    unsigned long long hp = 0, hn = 0, hist = 0;
    for (int i = 0; i < 6; i++) {
        hp += s.half_pos[i];
        hn += s.half_neg[i];
    }
    for (int i = 0; i < 64; i++) hist += s.history[i];
    std::printf("%s %d %llu %llu %016llx %016llx %016llx %016llx %016llx %d %d %d %d %d %u %u %u %u %u %u %d %d %d %d %d %d %d %d %llu %llu %llu\n", tag, c,
        static_cast<unsigned long long>(s.symbol_counter), static_cast<unsigned long long>(s.preamble_index), bits_of(s.tow_at_current_symbol),
        bits_of(s.tow), bits_of(s.tau_c), bits_of(s.tau_gps), bits_of(s.chip_acc), s.stat, s.crc_error_counter, s.history_size, s.prn, s.wn, s.t_k,
        s.t_b, s.previous_tb, s.n_t, s.n, s.n_4, s.frame_sync, s.ephemeris_str[0], s.ephemeris_str[1], s.ephemeris_str[2], s.ephemeris_str[3],
        s.utc_model_str_5, s.tow_set, s.tow_new, hp, hn, hist);
}

static std::unique_ptr<gnsship::Glonass_Gnav_Telemetry_Decoder_Hip> make(bool l2, int max_rounds, int C, const std::vector<int>& prns)
{
    std::unique_ptr<gnsship::Glonass_Gnav_Telemetry_Decoder_Hip> d;
    if (l2) d = std::make_unique<gnsship::Glonass_L2_Ca_Telemetry_Decoder_Hip>(gnsship::glonass_l2_ca_tlm_conf(max_rounds), C);
    else d = std::make_unique<gnsship::Glonass_L1_Ca_Telemetry_Decoder_Hip>(gnsship::glonass_l1_ca_tlm_conf(max_rounds), C);
    for (int c = 0; c < C; c++)
        if (!d->new_channel(c, prns[static_cast<size_t>(c)])) throw std::runtime_error("new_channel: " + d->last_error());
    return d;
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "confs") == 0) {
        const gnsship_gnav_conf a = gnsship::glonass_l1_ca_tlm_conf(2001), b = gnsship::glonass_l2_ca_tlm_conf(9999);
        std::printf("l1 max_rounds %d signal %d reserved %d strings_per_run %d size %zu state %zu\n", a.max_rounds, a.signal, a.reserved,
            GNSSHIP_GNAV_STRINGS_PER_RUN(a.max_rounds), sizeof(gnsship_gnav_string), sizeof(gnsship_gnav_state));
        std::printf("l2 max_rounds %d signal %d reserved %d strings_per_run %d size %zu state %zu\n", b.max_rounds, b.signal, b.reserved,
            GNSSHIP_GNAV_STRINGS_PER_RUN(b.max_rounds), sizeof(gnsship_gnav_string), sizeof(gnsship_gnav_state));
        return 0;
    }
    if (argc < 8 || std::strcmp(argv[1], "run") != 0) {
        std::fprintf(stderr, "usage: gnav_mirror_test confs | run FILE N C CUT l1|l2 PRN...\n");
        return 2;
    }
    const int n = std::atoi(argv[3]), C = std::atoi(argv[4]), cut = std::atoi(argv[5]);
    const bool l2 = std::strcmp(argv[6], "l2") == 0;
    if (n < 1 || n > 100000 || C < 2 || C > 64 || cut < 1 || argc != 7 + C || (!l2 && std::strcmp(argv[6], "l1") != 0)) return 2;
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
        auto dec = make(l2, cut, C, prns);
        int run = 0;
        for (int r = 0; r < n; r += cut, run++) {
            const int m = n - r < cut ? n - r : cut;
            if (run == 1 && !dec->set_satellite(0, 9)) return 1;
            if (!dec->work_symbols(sym.data() + static_cast<size_t>(r) * C, nullptr, nullptr, m)) {
                std::printf("work_symbols failed: %s\n", dec->last_error().c_str());
                return 1;
            }
            print_strings("str", *dec, C, false);
            for (int c = 0; c < C; c++) {
                uint32_t tow = 0, sf = 0;
                for (int k = 0; k < dec->rounds(); k++) {
                    tow += dec->tow_ms()[static_cast<size_t>(k) * C + c];
                    sf += dec->sflags()[static_cast<size_t>(k) * C + c];
                }
                std::printf("stream %d %d %u %u\n", run, c, tow, sf);
            }
        }
        for (int c = 0; c < C; c++) print_state("state", c, dec->state(c));
        std::printf("too_many %s\n", dec->work_symbols(sym.data(), nullptr, nullptr, cut + 1) ? "accepted" : "refused");
        std::printf("bad_channel %s\n", dec->new_channel(-1, 3) || dec->set_satellite(C, 3) || dec->set_state(C, dec->state(0)) ? "accepted" : "refused");
        std::printf("bad_prn %s\n", dec->set_satellite(0, 64) || dec->new_channel(0, -1) ? "accepted" : "refused");
        gnsship_gnav_state bad = dec->state(1);
        bad.stat = 3;
        std::printf("bad_state %s\n", dec->set_state(0, bad) ? "accepted" : "refused");
        if (!dec->set_state(0, dec->state(1))) return 1;
        print_state("copy", 0, dec->state(0));
        bool wrong_signal = false;
        try {
            gnsship::Glonass_L2_Ca_Telemetry_Decoder_Hip wrong(gnsship::glonass_l1_ca_tlm_conf(10), 1);
        } catch (const std::invalid_argument&) {
            wrong_signal = true;
        }
        std::printf("wrong_signal %s\n", wrong_signal ? "refused" : "accepted");

        // the same stream as tracking records: round 2r carries the symbol, round 2r + 1 an epoch that is no symbol
        auto rdec = make(l2, 2 * n, C, prns);
        std::vector<gnsship_trk_epoch> rec(static_cast<size_t>(2 * n) * C);
        std::memset(rec.data(), 0, rec.size() * sizeof(gnsship_trk_epoch));
        for (int r = 0; r < n; r++)
            for (int c = 0; c < C; c++) {
                gnsship_trk_epoch& e = rec[static_cast<size_t>(2 * r) * C + c];
                const double s = sym[static_cast<size_t>(r) * C + c];
                e.prompt_i = s;
                e.prompt_q = -s;
                e.flags = 9;
                e.sample_counter = 1000000ull + 4000ull * static_cast<uint64_t>(r) + static_cast<uint64_t>(c);
                gnsship_trk_epoch& skip = rec[static_cast<size_t>(2 * r + 1) * C + c];
                skip.prompt_i = skip.prompt_q = -s;
                skip.flags = 8;
            }
        if (!rdec->work_records(rec.data(), 2 * n)) {
            std::printf("work_records failed: %s\n", rdec->last_error().c_str());
            return 1;
        }
        print_strings("rstr", *rdec, C, true);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("gnav_mirror_test done\n");
    return 0;
}
