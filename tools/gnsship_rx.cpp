// gnsship_rx — standalone receiver core over the C ABI: File_Signal_Source → channels (acquisition →
// tracking, re-acquisition after a loss of lock) → per-channel tracking dumps, the Channel role of
// GNSS-SDR without GNU Radio (include/gnsship_receiver.hpp).  Keys mirror the reference's
// configuration (conf/gnss-sdr_GPS_L1_gr_complex.conf); GPS L1 C/A channels, or with --signal L5 GPS L5
// channels (acquisition on L5I, tracking on the L5Q pilot with the L5I data prompt), with --signal 2S GPS L2C
// channels (the L2 CM code, 20 ms epochs), with --signal B3 BeiDou B3I channels (a GEO satellite follows its PRN),
// with --signal 5X / 7X Galileo E5a / E5b channels (acquisition on the I component, tracking on the Q pilot with the I
// component on the data prompt; the records' symbols have I and Q exchanged, as the block hands them to telemetry).
//
//   gnsship_rx --file F [--item gr_complex|ishort|ibyte|float|short|byte|2bit|nsr|2bit-cpx|4bit-cpx]
//              [--sample-type real|iq|qi] [--big-endian-bytes] [--fs 4000000] [--seconds S] [--signal 1C|L5|2S|B3|5X|7X|1G|2G]
//              [--channels 5] [--in-acquisition 1] [--satellite CH:PRN ...] [--repeat-satellite]
//              [--pfa 0.01] [--doppler-max 10000] [--doppler-step 250]
//              [--pll-bw 40] [--dll-bw 4] [--order 3] [--pull-in-time-s 10] [--rotator auto|generic|avx]
//              [--max-carrier-lock-fail 5000] [--max-code-lock-fail 50] [--cn0-min 25]
//              [--block-ms 100] [--acq-piece 8192] [--dump PREFIX] [--events CSV] [--records BIN]
//              [--telemetry] [--telemetry-mode reference|full] [--lnav] [--cnav] [--dnav] [--gnav]
//              [--if-hz 0] [--decimation 1] [--filter-bw 0] [--filter-tw 0]
//              [--input-filter pulse-blanking|notch|notch-lite] [--input-filter-pfa P] [--segment-length 32]
//              [--segments-est 12500] [--segments-reset 5000000] [--p-c-factor 0.9] [--coeff-rate R]
//
// --telemetry (with --signal 5X or 7X) sends each tracking block's records through the device telemetry framing
// (F/NAV pages on 5X, I/NAV page parts on 7X) and prints, ahead of the summary, one line per page part: channel, PRN,
// symbol counter, even / odd, the CRC verdict as the block computes it, the bits as hex.  A telemetry fault goes back to
// the channel's tracking.  --telemetry-mode picks the Viterbi metric (reference: as the block; full: both symbols).
//
// --lnav (with --signal 1C) sends each tracking block's records through the device GPS L1 C/A telemetry decoder and
// prints, ahead of the summary, one line per emitted subframe: channel, PRN, symbol counter, subframe ID, TOW in seconds,
// ok / fail, the ten words as the block stores them in hex.  A telemetry fault goes back to the channel's tracking.
//
// --cnav (with --signal 2S or L5) sends each tracking block's records through the device GPS CNAV telemetry decoder and
// prints, ahead of the summary, one line per message (every 300-bit buffer a locked part disposed of): channel, PRN,
// symbol counter, the message's PRN, ID, TOW in 6-second units, alert, delay, part, ok / fail, the 38 bytes in hex; then per
// channel one "cnav-state" line with the decoder's members (the arrays as weighted sums, as tests/cpp/cnav_mirror_test
// prints them).  A telemetry fault goes back to the channel's tracking.
//
// --dnav (with --signal B3) sends each tracking block's records through the device BeiDou D1/D2 telemetry decoder and
// prints, ahead of the summary, one line per decoded subframe: channel, PRN, symbol counter, FraID, Pnum, SOW, the TOW in
// ms after the stamp, the corrected-rows mask and the flags in hex, the ten words in hex.
//
// --gnav (with --signal 1G or 2G) sends each tracking block's records through the device GLONASS GNAV telemetry decoder and
// prints, ahead of the summary, one line per decoded string: channel, the PRN the channel was assigned, the decoder's PRN
// after the decode (the slot number once string 4 has come), symbol and sample counter, string number, the flipped bit or
// -1, the TOW in ms of that symbol, d_TOW, the flags in hex and the 85 bits as three words in hex.
//
// --input-filter puts the interference mitigation (InputFilter.implementation = Pulse_Blanking_Filter, Notch_Filter or
// Notch_Filter_Lite; pfa, length, segments_est, segments_reset, p_c_factor, coeff_rate: 0 = the adapter's defaults)
// on the device ahead of the channels: on the conditioned band with --if-hz / --decimation, else on the gr_complex
// file itself.  Its pfa is --input-filter-pfa, as --pfa is the acquisition's.
//
// --if-hz / --decimation (either one) put the signal conditioner ahead of the channels (InputFilter.implementation =
// Freq_Xlating_Fir_Filter, filter_type lowpass: IF, decimation_factor, bw, tw; 0 = the adapter's defaults): the file is
// read at --fs and goes to the device as it is, acquisition and tracking run on the conditioned stream at fs / decimation.
// The receiver core brings every conditioned block back to the host (its acquisition blocks buffer their dwells there)
// and uploads the tracking window again: one device-to-host and one host-to-device copy of the conditioned block per block.
//
// ishort / ibyte samples are converted to gr_complex without scaling (Ishort_To_Complex /
// Ibyte_To_Complex, item_type_helpers.cc:27-73).
//
// --item float|short|byte is a real-sampled IF stream (the Freq_Xlating_Fir_Filter adapter's input_item_type).  The
// packed items are the byte files of the reference's packed sources: 2bit = Two_Bit_Packed_File_Signal_Source
// (--sample-type real|iq|qi, default real; --big-endian-bytes), nsr = Nsr_File_Signal_Source (real), 2bit-cpx =
// Two_Bit_Cpx_File_Signal_Source, 4bit-cpx = Four_Bit_Cpx_File_Signal_Source (--sample-type iq|qi, default iq).
// With the conditioner on they go to the device as they are (GNSSHIP_FMT_*).  Real items need the conditioner
// (--if-hz / --decimation); packed complex items without it are unpacked to gr_complex here, as ishort / ibyte are.
// stdout: one JSON summary line.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "gnsship_receiver.hpp"

namespace {

[[noreturn]] void usage(const char* why)
{
    std::fprintf(stderr, "gnsship_rx: %s\n", why);
    std::exit(2);
}

// Field j (stream order) of a byte of a packed format, value map applied (GNSSHIP_FMT_PACKED, include/gnsship.h).
float packed_field(uint8_t byte, int j, int fmt)
{
    const int bits = GNSSHIP_FMT_PACKED_BITS(fmt);
    const int off = GNSSHIP_FMT_PACKED_ORDER(fmt) == GNSSHIP_FMT_PACKED_MSB_FIRST ? 8 - bits * (j + 1) : bits * j;
    int s = (byte >> off) & ((1 << bits) - 1);
    if (s >= (1 << (bits - 1))) s -= 1 << bits;
    return static_cast<float>(GNSSHIP_FMT_PACKED_MAP(fmt) == GNSSHIP_FMT_PACKED_MAP_2S1 ? 2 * s + 1 : s);
}

}  // namespace

int main(int argc, char** argv)
{
    std::string file, item = "gr_complex", sample_type, dump, events_csv, records_bin, rotator = "auto", signal = "1C";
    double fs = 4e6, seconds = 0.0, block_ms = 100.0;
    double if_hz = 0.0, filter_bw = 0.0, filter_tw = 0.0;
    int decimation = 1;
    bool conditioner = false, big_endian_bytes = false;
    std::string mit;
    double mit_pfa = 0.0, mit_p_c = 0.9, mit_coeff_rate = 0.0;
    int mit_length = 32, mit_est = 12500, mit_reset = 5000000;
    gnsship::Receiver_Conf rc;
    rc.channels = 5;
    rc.in_acquisition = 1;
    rc.acq.pfa = 0.01F;
    rc.acq.doppler_max = 10000;
    rc.acq.doppler_step = 250.0F;
    rc.trk.pll_bw_hz = 40.0F;
    rc.trk.dll_bw_hz = 4.0F;
    rc.trk.pll_filter_order = 3;
    std::vector<std::pair<int, unsigned>> sats;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string {
            if (i + 1 >= argc) usage(("missing value for " + a).c_str());
            return argv[++i];
        };
        if (a == "--file") file = val();
        else if (a == "--item") item = val();
        else if (a == "--sample-type") sample_type = val();
        else if (a == "--big-endian-bytes") big_endian_bytes = true;
        else if (a == "--signal") signal = val();
        else if (a == "--fs") fs = std::atof(val().c_str());
        else if (a == "--seconds") seconds = std::atof(val().c_str());
        else if (a == "--channels") rc.channels = std::atoi(val().c_str());
        else if (a == "--in-acquisition") rc.in_acquisition = std::atoi(val().c_str());
        else if (a == "--satellite") {
            const std::string v = val();
            const size_t k = v.find(':');
            if (k == std::string::npos) usage("--satellite wants CH:PRN");
            sats.push_back({std::atoi(v.substr(0, k).c_str()), static_cast<unsigned>(std::atoi(v.substr(k + 1).c_str()))});
        } else if (a == "--repeat-satellite") rc.repeat_satellite = true;
        else if (a == "--pfa") rc.acq.pfa = static_cast<float>(std::atof(val().c_str()));
        else if (a == "--threshold") rc.threshold = static_cast<float>(std::atof(val().c_str()));
        else if (a == "--doppler-max") rc.acq.doppler_max = std::atoi(val().c_str());
        else if (a == "--doppler-step") rc.acq.doppler_step = static_cast<float>(std::atof(val().c_str()));
        else if (a == "--pll-bw") rc.trk.pll_bw_hz = static_cast<float>(std::atof(val().c_str()));
        else if (a == "--dll-bw") rc.trk.dll_bw_hz = static_cast<float>(std::atof(val().c_str()));
        else if (a == "--order") rc.trk.pll_filter_order = std::atoi(val().c_str());
        else if (a == "--pull-in-time-s") rc.trk.pull_in_time_s = static_cast<uint32_t>(std::atoi(val().c_str()));
        else if (a == "--max-carrier-lock-fail") rc.trk.max_carrier_lock_fail = std::atoi(val().c_str());  // gflags (gnss_sdr_flags.cc)
        else if (a == "--max-code-lock-fail") rc.trk.max_code_lock_fail = std::atoi(val().c_str());
        else if (a == "--cn0-min") rc.trk.cn0_min = std::atoi(val().c_str());
        else if (a == "--rotator") rotator = val();
        else if (a == "--block-ms") block_ms = std::atof(val().c_str());
        else if (a == "--acq-piece") rc.acq_piece = std::atoi(val().c_str());
        else if (a == "--if-hz") {
            if_hz = std::atof(val().c_str());
            conditioner = true;
        } else if (a == "--decimation") {
            decimation = std::atoi(val().c_str());
            conditioner = true;
        } else if (a == "--filter-bw") filter_bw = std::atof(val().c_str());
        else if (a == "--filter-tw") filter_tw = std::atof(val().c_str());
        else if (a == "--input-filter") mit = val();
        else if (a == "--input-filter-pfa") mit_pfa = std::atof(val().c_str());
        else if (a == "--segment-length") mit_length = std::atoi(val().c_str());
        else if (a == "--segments-est") mit_est = std::atoi(val().c_str());
        else if (a == "--segments-reset") mit_reset = std::atoi(val().c_str());
        else if (a == "--p-c-factor") mit_p_c = std::atof(val().c_str());
        else if (a == "--coeff-rate") mit_coeff_rate = std::atof(val().c_str());
        else if (a == "--dump") dump = val();
        else if (a == "--events") events_csv = val();
        else if (a == "--records") records_bin = val();
        else if (a == "--telemetry") rc.telemetry = true;
        else if (a == "--lnav") rc.lnav = true;
        else if (a == "--cnav") rc.cnav = true;
        else if (a == "--dnav") rc.dnav = true;
        else if (a == "--gnav") rc.gnav = true;
        else if (a == "--telemetry-mode") {
            const std::string m = val();
            if (m != "reference" && m != "full") usage("--telemetry-mode must be reference or full");
            rc.telemetry_mode = m == "full" ? GNSSHIP_VIT_MODE_FULL : GNSSHIP_VIT_MODE_REFERENCE;
        }
        else usage(("unknown option " + a).c_str());
    }
    if (file.empty()) usage("--file is required");
    int fmt = -1;
    if (item == "gr_complex") fmt = GNSSHIP_FMT_CF32;
    else if (item == "ishort") fmt = GNSSHIP_FMT_CI16;
    else if (item == "ibyte") fmt = GNSSHIP_FMT_CI8;
    else if (item == "float") fmt = GNSSHIP_FMT_RF32;
    else if (item == "short") fmt = GNSSHIP_FMT_RI16;
    else if (item == "byte") fmt = GNSSHIP_FMT_RI8;
    else if (item == "2bit") {
        gnsship::Two_Bit_Packed_File_Signal_Source_Conf src;
        if (!sample_type.empty()) src.sample_type = sample_type;
        src.big_endian_bytes = big_endian_bytes;
        fmt = src.format();
        if (fmt < 0) usage("--sample-type must be real, iq or qi with --item 2bit");
    } else if (item == "nsr") fmt = gnsship::Nsr_File_Signal_Source_Conf().format();
    else if (item == "2bit-cpx") fmt = gnsship::Two_Bit_Cpx_File_Signal_Source_Conf().format();
    else if (item == "4bit-cpx") {
        gnsship::Four_Bit_Cpx_File_Signal_Source_Conf src;
        if (!sample_type.empty()) src.sample_type = sample_type;
        fmt = src.format();
        if (fmt < 0) usage("--sample-type must be iq or qi with --item 4bit-cpx");
    } else usage("--item must be gr_complex, ishort, ibyte, float, short, byte, 2bit, nsr, 2bit-cpx or 4bit-cpx");
    if ((!sample_type.empty() || big_endian_bytes) && item != "2bit" && !(item == "4bit-cpx" && !big_endian_bytes))
        usage("--sample-type goes with --item 2bit or 4bit-cpx, --big-endian-bytes with --item 2bit");
    const bool packed = GNSSHIP_FMT_IS_PACKED(fmt);
    const bool real_items = fmt == GNSSHIP_FMT_RF32 || fmt == GNSSHIP_FMT_RI16 || fmt == GNSSHIP_FMT_RI8 ||
                            (packed && GNSSHIP_FMT_PACKED_COMPONENTS(fmt) == GNSSHIP_FMT_PACKED_REAL);
    if (real_items && !conditioner) usage("real-sampled items need the conditioner (--if-hz / --decimation)");
    const int64_t sample_bits = gnsship_cond_fmt_bits(fmt);
    const int64_t per_byte = sample_bits < 8 ? 8 / sample_bits : 1;  // samples per byte of a packed item
    if (signal != "1C" && signal != "L5" && signal != "2S" && signal != "B3" && signal != "5X" && signal != "7X" && signal != "1G" && signal != "2G")
        usage("--signal must be 1C, L5, 2S, B3, 5X, 7X, 1G or 2G");
    if (rc.lnav && signal != "1C") usage("--lnav decodes GPS L1 C/A channels (--signal 1C)");
    if (rc.cnav && signal != "2S" && signal != "L5") usage("--cnav decodes GPS L2C or L5 channels (--signal 2S or L5)");
    if (rc.dnav && signal != "B3") usage("--dnav decodes BeiDou B3I channels (--signal B3)");
    if (rc.gnav && signal != "1G" && signal != "2G") usage("--gnav decodes GLONASS channels (--signal 1G or 2G)");
    std::snprintf(rc.trk.signal, sizeof(rc.trk.signal), "%s", signal.c_str());
    if (signal == "B3") rc.trk.system = 'C';  // otherwise 'G'
    if (signal == "5X" || signal == "7X") rc.trk.system = 'E';
    if (signal == "1G" || signal == "2G") rc.trk.system = 'R';  // GLONASS: each PRN acquired under its own channel's bias
    const double fs_file = fs;  // the rate the file is read at; fs from here on is the channels' rate
    if (conditioner) {
        if (decimation < 1 || std::fmod(fs, static_cast<double>(decimation)) != 0.0) usage("--decimation must divide --fs");
        if (fs != std::floor(fs) || if_hz != std::floor(if_hz)) usage("--fs and --if-hz must be whole numbers of Hz with the conditioner on");
        int n_taps = 0;  // the adapter's low-pass design, checked before the device is touched
        if (filter_bw < 0.0 || filter_tw < 0.0 || gnsship_cond_lowpass_taps(fs, decimation, filter_bw, filter_tw, nullptr, 0, &n_taps) != GNSSHIP_OK)
            usage("--filter-bw must lie in (0, fs/2] and --filter-tw be positive (0 = the adapter's defaults)");
        if (n_taps > GNSSHIP_COND_MAX_TAPS) usage("--filter-tw gives more than 4096 taps");
        rc.use_conditioner = true;
        rc.input_filter.IF = if_hz;
        rc.input_filter.sampling_frequency = fs_file;
        rc.input_filter.decimation_factor = decimation;
        rc.input_filter.filter_type = "lowpass";
        rc.input_filter.bw = filter_bw;
        rc.input_filter.tw = filter_tw;
        fs = fs_file / decimation;
    }
    if (!mit.empty()) {
        if (mit != "pulse-blanking" && mit != "notch" && mit != "notch-lite") usage("--input-filter must be pulse-blanking, notch or notch-lite");
        if (!conditioner && item != "gr_complex") usage("--input-filter reads gr_complex items, or the conditioned band (--if-hz / --decimation)");
        if (mit_length < 2 || mit_length > GNSSHIP_MIT_MAX_LENGTH || mit_est < 1 || mit_pfa < 0.0 || mit_pfa >= 1.0)
            usage("--segment-length in 2..1024, --segments-est >= 1, --input-filter-pfa in (0, 1)");
        rc.mitigation = mit == "pulse-blanking" ? "Pulse_Blanking_Filter" : mit == "notch" ? "Notch_Filter" : "Notch_Filter_Lite";
        if (mit_pfa > 0.0) rc.pulse_blanking.pfa = rc.notch.pfa = rc.notch_lite.pfa = static_cast<float>(mit_pfa);
        rc.pulse_blanking.length = rc.notch.length = rc.notch_lite.length = mit_length;
        rc.pulse_blanking.segments_est = rc.notch.segments_est = rc.notch_lite.segments_est = mit_est;
        rc.pulse_blanking.segments_reset = rc.notch.segments_reset = rc.notch_lite.segments_reset = mit_reset;
        rc.notch.p_c_factor = rc.notch_lite.p_c_factor = static_cast<float>(mit_p_c);
        rc.notch_lite.sampling_frequency = static_cast<float>(fs);  // the rate the filter runs at
        rc.notch_lite.coeff_rate = static_cast<float>(mit_coeff_rate);
    }
    rc.acq.fs_in = static_cast<int64_t>(fs);
    rc.trk.fs_in = fs;
    // gps_l1_ca_dll_pll_tracking.cc:47, gps_l5_dll_pll_tracking.cc:47, beidou_b3i_dll_pll_tracking.cc:47; gps_l2_m_dll_pll_tracking.cc:47
    rc.trk.vector_length = static_cast<uint32_t>(std::lround(fs / (signal == "2S" ? 50.0 : 1000.0)));
    rc.trk.rotator = rotator == "generic" ? GNSSHIP_ROTATOR_GENERIC : rotator == "avx" ? GNSSHIP_ROTATOR_AVX : GNSSHIP_ROTATOR_AUTO;
    // the GLONASS block's correlator has the generic rotator only: "auto" means that one here, "avx" is refused by the engine
    if ((signal == "1G" || signal == "2G") && rotator == "auto") rc.trk.rotator = GNSSHIP_ROTATOR_GENERIC;
    rc.block_samples = static_cast<int64_t>(fs * block_ms / 1000.0);
    rc.dump_filename = dump;
    rc.satellite.assign(static_cast<size_t>(rc.channels), 0U);
    for (const auto& s : sats)
        if (s.first >= 0 && s.first < rc.channels) rc.satellite[static_cast<size_t>(s.first)] = s.second;

    std::FILE* f = std::fopen(file.c_str(), "rb");
    if (!f) usage(("cannot open " + file).c_str());
    if (!dump.empty())
        for (int c = 0; c < rc.channels; c++) std::remove((dump + std::to_string(c) + ".dat").c_str());

    const auto t_init = std::chrono::steady_clock::now();
    std::unique_ptr<gnsship::Gnss_Receiver_Hip> rxp;
    try {
        rxp = std::make_unique<gnsship::Gnss_Receiver_Hip>(rc);
    } catch (const std::invalid_argument& e) {  // a configuration the engines refuse
        usage(e.what());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "gnsship_rx: %s\n", e.what());
        return 1;
    }
    gnsship::Gnss_Receiver_Hip& rx = *rxp;
    const int64_t block = (rc.block_samples > 0 ? rc.block_samples : static_cast<int64_t>(fs / 10)) * decimation;  // file samples
    const int64_t limit = seconds > 0 ? static_cast<int64_t>(seconds * fs_file) : INT64_MAX;
    int64_t unit = conditioner ? decimation : 1;  // samples handed on at a time: whole conditioned samples, whole bytes
    while (unit % per_byte != 0) unit += conditioner ? decimation : 1;
    std::vector<char> raw(static_cast<size_t>((block * sample_bits + 7) / 8));
    std::vector<std::complex<float>> x(static_cast<size_t>(block));
    int64_t total = 0;
    double io_s = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    while (total < limit) {
        const auto r0 = std::chrono::steady_clock::now();
        int64_t want = std::min<int64_t>(block, limit - total);
        want -= want % per_byte;
        size_t got = static_cast<size_t>(static_cast<int64_t>(std::fread(raw.data(), 1, static_cast<size_t>(want * sample_bits / 8), f)) * 8 / sample_bits);
        got -= got % static_cast<size_t>(unit);  // a whole number of conditioned samples and of bytes
        if (got == 0) break;
        if (conditioner || !mit.empty()) {
            io_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - r0).count();
            if (!rx.work_raw(raw.data(), fmt, static_cast<int64_t>(got))) {
                std::fprintf(stderr, "gnsship_rx: input filter / engine error\n");
                return 1;
            }
            total += static_cast<int64_t>(got);
            continue;
        }
        if (item == "gr_complex") {
            std::memcpy(x.data(), raw.data(), got * 8);
        } else if (packed) {  // a complex packed item (real ones need the conditioner)
            const uint8_t* s = reinterpret_cast<const uint8_t*>(raw.data());
            const int re = GNSSHIP_FMT_PACKED_COMPONENTS(fmt) == GNSSHIP_FMT_PACKED_QI ? 1 : 0;
            for (size_t i = 0; i < got; i++) {
                const uint8_t b = s[i / static_cast<size_t>(per_byte)];
                const int j = 2 * static_cast<int>(i % static_cast<size_t>(per_byte));
                x[i] = {packed_field(b, j + re, fmt), packed_field(b, j + 1 - re, fmt)};
            }
        } else if (item == "ishort") {
            const int16_t* s = reinterpret_cast<const int16_t*>(raw.data());
            for (size_t i = 0; i < got; i++) x[i] = {static_cast<float>(s[2 * i]), static_cast<float>(s[2 * i + 1])};
        } else {
            const int8_t* s = reinterpret_cast<const int8_t*>(raw.data());
            for (size_t i = 0; i < got; i++) x[i] = {static_cast<float>(s[2 * i]), static_cast<float>(s[2 * i + 1])};
        }
        io_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - r0).count();
        if (!rx.work(x.data(), static_cast<int64_t>(got))) {
            std::fprintf(stderr, "gnsship_rx: engine error\n");
            return 1;
        }
        total += static_cast<int64_t>(got);
    }
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const double init_s = std::chrono::duration<double>(t0 - t_init).count();
    std::fclose(f);

    if (!events_csv.empty()) {
        std::FILE* e = std::fopen(events_csv.c_str(), "w");
        if (e) {
            std::fprintf(e, "sample,channel,what,prn,doppler_hz,delay_samples,test_statistic\n");
            for (const auto& ev : rx.events())
                std::fprintf(e, "%llu,%d,%d,%u,%.17g,%.17g,%.9g\n", static_cast<unsigned long long>(ev.sample), ev.channel, ev.what, ev.prn, ev.doppler_hz,
                    ev.delay_samples, static_cast<double>(ev.test_statistic));
            std::fclose(e);
        }
    }
    if (!records_bin.empty()) {  // per record: int32 channel, int32 prn, then the gnsship_trk_epoch
        std::FILE* r = std::fopen(records_bin.c_str(), "wb");
        if (r) {
            for (int c = 0; c < rc.channels; c++)
                if (c < static_cast<int>(rx.records().size()))
                    for (const auto& e : rx.records()[static_cast<size_t>(c)]) {
                        const int32_t hdr[2] = {c, static_cast<int32_t>(e.prn)};
                        std::fwrite(hdr, sizeof(hdr), 1, r);
                        std::fwrite(&e.e, sizeof(e.e), 1, r);
                    }
            std::fclose(r);
        }
    }
    // --telemetry: one line per page part — channel, PRN, symbol counter, even / odd / page, CRC verdict, the bits as hex
    for (const auto& pg : rx.pages()) {
        std::string hex;
        for (size_t i = 0; i < pg.bits.size(); i += 4) {
            int v = 0;
            for (size_t j = 0; j < 4; j++) v = (v << 1) | (i + j < pg.bits.size() ? pg.bits[i + j] : 0);
            hex += "0123456789abcdef"[v];
        }
        std::printf("page channel %d prn %u symbol %llu %s crc %s %s\n", pg.page.channel, pg.prn, static_cast<unsigned long long>(pg.page.symbol_counter),
            signal == "7X" ? ((pg.page.flags & 8) ? "odd" : "even") : "page", (pg.page.flags & 1) ? "ok" : "fail", hex.c_str());
    }
    // --lnav: one line per emitted subframe — channel, PRN, symbol counter, ID, TOW, the decode's verdict, the ten words
    for (const auto& sf : rx.subframes()) {
        std::printf("subframe channel %d prn %u symbol %llu id %d tow %u %s", sf.subframe.channel, sf.prn,
            static_cast<unsigned long long>(sf.subframe.symbol_counter), sf.subframe.subframe_id, sf.subframe.tow_s, (sf.subframe.flags & 1) ? "ok" : "fail");
        for (int w = 0; w < 10; w++) std::printf(" %08x", sf.subframe.words[w]);
        std::printf("\n");
    }
    // --cnav: one line per message — channel, PRN, symbol counter, the message's fields, the CRC verdict, the 38 bytes;
    // then each channel's decoder members
    for (const auto& cm : rx.cnav_messages()) {
        const gnsship_cnav_message& m = cm.message;
        std::printf("message channel %d prn %u symbol %llu msg_prn %u id %u tow %u alert %u delay %u part %u %s ", m.channel, cm.prn,
            static_cast<unsigned long long>(m.symbol_counter), m.prn, m.msg_id, m.tow, m.alert, m.delay, m.part, (m.flags & 1) ? "ok" : "fail");
        for (int b = 0; b < 38; b++) std::printf("%02x", m.raw[b]);
        std::printf("\n");
    }
    for (int c = 0; rx.has_cnav() && c < rc.channels; c++) {
        const gnsship_cnav_state s = rx.cnav_state(c);
        std::printf("cnav-state %d %llu %llu %.17g %u %u %d %d %d", c, static_cast<unsigned long long>(s.symbol_counter),
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
    // --gnav: one line per decoded string
    for (const auto& gs : rx.gnav_strings()) {
        const gnsship_gnav_string& f = gs.string;
        std::printf("gnav-string channel %d prn %u slot %d symbol %llu sample %llu string %d flipped %d tow_ms %u tow %.17g flags %02x bits %08x %08x %08x\n",
            f.channel, gs.prn, f.prn, static_cast<unsigned long long>(f.symbol_counter), static_cast<unsigned long long>(f.sample_counter), f.string_id,
            f.flipped_bit, f.tow_at_current_symbol_ms, f.tow, f.flags, f.bits[0], f.bits[1], f.bits[2]);
    }
    // --dnav: one line per decoded subframe
    for (const auto& ds : rx.dnav_subframes()) {
        const gnsship_dnav_subframe& f = ds.subframe;
        std::printf("dnav-subframe channel %d prn %u symbol %llu fraid %d pnum %d sow %u tow_ms %u corrected %05x flags %02x", f.channel, ds.prn,
            static_cast<unsigned long long>(f.symbol_counter), f.fra_id, f.pnum, f.sow, f.tow_at_current_symbol_ms, f.corrected_mask, f.flags);
        for (int w = 0; w < 10; w++) std::printf(" %08x", f.words[w]);
        std::printf("\n");
    }
    int n_pos = 0, n_neg = 0, n_lost = 0;
    for (const auto& ev : rx.events()) {
        n_pos += ev.what == 1;
        n_neg += ev.what == 0;
        n_lost += ev.what == 2;
    }
    std::printf("{\"samples\": %lld, \"signal_s\": %.6f, \"wall_s\": %.6f, \"init_s\": %.6f, \"io_s\": %.6f, \"realtime_factor\": %.3f, "
                "\"acq_positive\": %d, \"acq_negative\": %d, \"losses\": %d, \"channels\": [",
        static_cast<long long>(total), static_cast<double>(total) / fs_file, wall, init_s, io_s, (static_cast<double>(total) / fs_file) / wall, n_pos, n_neg,
        n_lost);
    for (int c = 0; c < rc.channels; c++) {
        const size_t nr = c < static_cast<int>(rx.records().size()) ? rx.records()[static_cast<size_t>(c)].size() : 0;
        std::printf("%s{\"channel\": %d, \"prn\": %u, \"fsm_state\": %u, \"tracking_state\": %d, \"epochs\": %zu}", c ? ", " : "", c, rx.channel_prn(c),
            rx.channel_fsm_state(c), rx.tracking_state(c), nr);
    }
    std::printf("]}\n");
    return 0;
}
