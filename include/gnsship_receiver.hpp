// gnsship_receiver.hpp — the Channel role over the C ABI: a standalone receiver core that reads an IF
// stream, acquires, hands off to tracking and re-acquires after a loss of lock, the way GNSS-SDR's
// flowgraph drives its channels — without GNU Radio (absent here).
//
// Reference pieces restated (paths relative to the reference root):
//   ChannelFsm                  src/algorithms/channel/libs/channel_fsm.cc:44-220 (states 0 standby,
//                               1 acquisition, 2 tracking, 3 waiting for a satellite; the events)
//   channel_msg_receiver_cc     src/algorithms/channel/libs/channel_msg_receiver_cc.cc:64-100 (acquisition
//                               positive / negative, tracking loss → FSM events; repeat_satellite)
//   Channel                     src/algorithms/channel/adapters/channel.cc:30-108, :215-275 (set_signal →
//                               set_local_code, start_acquisition, assist_acquisition_doppler)
//   GNSSFlowgraph control       src/core/receiver/gnss_flowgraph.cc: set_channels_state :2540-2564,
//                               acquisition_manager :1797-1879, apply_action :1904-2009 (what 0/1/2),
//                               search_next_signal :2615-2629 (GPS 1C), push_back_signal :1652-1660,
//                               remove_signal :1718-1724, set_signals_list :2158-2170 (GPS PRN 1-32)
//   the blocks                  Pcps_Acquisition_Hip::general_work (pcps_acquisition.cc:902-1031) and
//                               Dll_Pll_Veml_Tracking_Hip (dll_pll_veml_tracking.cc) from gnsship_cpp.hpp
//
// Scheduling model (deterministic, one host thread): the stream is processed in blocks.  Within a
// block every channel in acquisition runs its general_work over pieces of `acq_piece` samples (GNU
// Radio's noutput) in stream order; a decision takes effect at the sample where it was made (a positive
// acquisition starts tracking there; a failure hands the next satellite to the next idle channel,
// whose acquisition starts there).  Then the tracking engine runs every tracking channel over the
// block on the device (the closed loop of gnsship_trk_*; each channel continues exactly where it
// stopped, the last 2·vector_length samples of the previous block are kept in front).  A loss of
// lock found in a block re-starts that channel's acquisition at the next block: the control thread's
// reaction latency is one block.  An inactive acquisition consumes the stream as the reference block
// does (its sample counter, hence Acq_samplestamp_samples, is the absolute stream position).
#ifndef GNSSHIP_RECEIVER_HPP
#define GNSSHIP_RECEIVER_HPP

#include <algorithm>
#include <cstdint>
#include <functional>
#include <list>
#include <memory>
#include <string>
#include <vector>

#include "gnsship_cpp.hpp"

namespace gnsship {

// ChannelFsm (channel_fsm.cc:44-220).  The actions are the adapters' calls and the control-queue pushes.
class ChannelFsm {
public:
    std::function<void()> start_acquisition, stop_acquisition, start_tracking, stop_tracking, request_satellite, notify_stop_tracking;
    bool Event_stop_channel()
    {
        if (state_ == 1) {
            state_ = 0;
            stop_acquisition();
        } else if (state_ == 2) {
            state_ = 0;
            stop_tracking();
        }
        return true;
    }
    bool Event_start_acquisition()
    {
        if (state_ == 1 || state_ == 2) return false;
        state_ = 1;
        start_acquisition();
        return true;
    }
    bool Event_valid_acquisition()
    {
        if (state_ != 1) return false;
        state_ = 2;
        start_tracking();
        return true;
    }
    bool Event_failed_acquisition_repeat()
    {
        if (state_ != 1) return false;
        state_ = 1;
        start_acquisition();
        return true;
    }
    bool Event_failed_acquisition_no_repeat()
    {
        if (state_ != 1) return false;
        state_ = 3;
        request_satellite();
        return true;
    }
    bool Event_failed_tracking_standby()
    {
        if (state_ != 2) return false;
        state_ = 0;
        notify_stop_tracking();
        return true;
    }
    unsigned state() const { return state_; }

private:
    unsigned state_ = 0;
};

// The configuration keys of the 1C channels (conf/gnss-sdr_GPS_L1_gr_complex.conf); with trk.signal = "L5"
// the same keys of the L5 channels (Channels_L5, Acquisition_L5, Tracking_L5), with "2S" of the L2C channels
// (Channels_2S, ...; vector_length = round(fs / 50)), with trk.system 'C' and trk.signal "B3" of the BeiDou B3I ones,
// with trk.system 'E' and trk.signal "5X" / "7X" of the Galileo E5a / E5b ones, with trk.system 'R' and trk.signal "1G" / "2G"
// (trk = glonass_l1_ca_trk_conf / glonass_l2_ca_trk_conf) of the GLONASS L1 / L2 C/A ones.
struct Receiver_Conf {
    int channels{1};                     // Channels_1C.count
    int in_acquisition{1};               // Channels.in_acquisition (capped at channels)
    std::vector<uint32_t> satellite;     // Channel<i>.satellite (0 or missing: from the search list)
    bool repeat_satellite{false};        // Acquisition_1C.repeat_satellite
    Acq_Conf acq;                        // Acquisition_1C.* (pfa > 0: threshold from calculate_threshold)
    float threshold{0.0F};               // Acquisition_1C.threshold (used when pfa = 0)
    Dll_Pll_Conf trk;                    // Tracking_1C.* (vector_length = round(fs / 1000))
    int64_t block_samples{0};            // processing block (0: 100 ms of samples)
    int acq_piece{8192};                 // samples per acquisition general_work call
    std::string dump_filename;           // Tracking_1C.dump_filename ("" = dump off)
    int device{0};
    // Optional Signal_Conditioner ahead of the channels (gnss_flowgraph.cc:1008-1140) with InputFilter.implementation =
    // Freq_Xlating_Fir_Filter (conf/gnss-sdr_BDS_B3I_GPS_L1_CA_ibyte.conf:41-96): the source's samples enter through
    // work_raw() at input_filter.sampling_frequency, the channels run on the conditioned stream, so acq.fs_in and
    // trk.fs_in are sampling_frequency / decimation_factor and the channels' own IF is 0.  Off: exactly the receiver above.
    bool use_conditioner{false};
    Freq_Xlating_Fir_Filter_Conf input_filter;   // InputFilter.*
    // Optional interference mitigation, the InputFilter.implementation choices Pulse_Blanking_Filter, Notch_Filter and
    // Notch_Filter_Lite ("" = none): runs on the device on the conditioned band, or on a raw gr_complex stream when
    // no conditioner is configured, before the block goes to the host.  The samples enter through work_raw().
    std::string mitigation;
    Pulse_Blanking_Filter_Conf pulse_blanking;
    Notch_Filter_Conf notch;
    Notch_Filter_Lite_Conf notch_lite;
    // Optional telemetry framing on the device (galileo_telemetry_decoder_gs up to the CRC; Galileo_Telemetry_Decoder_Hip),
    // Galileo channels only: "5X" decodes F/NAV pages, "7X" I/NAV page parts.  Each tracking block's records go through
    // the decoder where tracking left them on the device; a channel whose check_tlm_separation fires gets the fault message
    // of msg_handler_telemetry_to_trk.  Off (the default): exactly the receiver above, every output byte for byte.
    bool telemetry{false};
    int telemetry_mode{GNSSHIP_VIT_MODE_REFERENCE};  // GNSSHIP_VIT_MODE_*
    // Optional GPS L1 C/A telemetry on the device (gps_l1_ca_telemetry_decoder_gs up to the time of week;
    // Gps_L1_Ca_Telemetry_Decoder_Hip), 1C channels only.  Each tracking block's records go through the decoder where
    // tracking left them on the device; a channel that is assigned a satellite gets a new block object; a channel whose
    // check_tlm_separation fires gets the fault message of msg_handler_telemetry_to_trk.  Off (the default): exactly the
    // receiver above, every output byte for byte.
    bool lnav{false};
    // Optional GPS CNAV telemetry on the device (gps_l2c_telemetry_decoder_gs / gps_l5_telemetry_decoder_gs up to the time
    // of week; Gps_L2c_Telemetry_Decoder_Hip / Gps_L5_Telemetry_Decoder_Hip), 2S and L5 channels only.  Each tracking
    // block's records go through the decoder where tracking left them on the device; a channel that is assigned a
    // satellite gets a new block object; a channel whose watchdog fires gets the fault message of
    // msg_handler_telemetry_to_trk.  Off (the default): exactly the receiver above, every output byte for byte.
    bool cnav{false};
    // Optional BeiDou D1/D2 telemetry on the device (beidou_b3i_telemetry_decoder_gs up to the time of week;
    // Beidou_B3i_Telemetry_Decoder_Hip), B3 channels only (the receiver has no B1I channels).  Each tracking block's
    // records go through the decoder where tracking left them on the device; a channel that is assigned a satellite gets a
    // new block object on that PRN.  The blocks publish nothing to tracking, so nothing goes back.  Off (the default):
    // exactly the receiver above, every output byte for byte.
    bool dnav{false};
    // Decode the GLONASS GNAV telemetry of every channel on the device (gnsship_cpp.hpp Glonass_L1_Ca_Telemetry_Decoder_Hip /
    // Glonass_L2_Ca_Telemetry_Decoder_Hip), system 'R' channels only.  Each tracking block's records go through the decoder
    // where tracking left them on the device; a channel that is assigned a satellite gets a new block object on that PRN,
    // and after string 4 the decoder's PRN is the slot number the satellite sent (the record's prn, gnav_prn()).  The blocks
    // publish nothing to tracking, so nothing goes back.  Off (the default): exactly the receiver above, byte for byte.
    bool gnav{false};
};

// One control event, in stream order.
struct Receiver_Event {
    uint64_t sample;   // stream position where it took effect
    int channel;
    int what;          // 0 acquisition failed, 1 acquisition positive, 2 tracking lost, 3 acquisition started
    uint32_t prn;
    double doppler_hz, delay_samples;  // acquisition outcome (what 0/1)
    float test_statistic;
};

// One tracking epoch of a channel with the satellite it was tracking (Gnss_Synchro::PRN).
struct Receiver_Record {
    uint32_t prn;
    gnsship_trk_epoch e;
};

// One decoded page part of a channel with the satellite it was tracking.
struct Receiver_Page {
    uint32_t prn;
    gnsship_tlm_page page;
    std::vector<uint8_t> bits;  // bytes of 0 / 1: 114 (I/NAV part) or 238 (F/NAV page)
};

// One LNAV subframe of a channel with the satellite it was tracking.
struct Receiver_Subframe {
    uint32_t prn;
    gnsship_lnav_subframe subframe;
};

// One CNAV message of a channel (every 300-bit buffer a locked part disposed of) with the satellite it was tracking.
struct Receiver_Cnav_Message {
    uint32_t prn;
    gnsship_cnav_message message;
};

// One BeiDou D1/D2 subframe of a channel (every decode) with the satellite it was tracking.
struct Receiver_Dnav_Subframe {
    uint32_t prn;
    gnsship_dnav_subframe subframe;
};

// One GLONASS GNAV string of a channel (every decode) with the satellite the channel was assigned; string.prn is the
// decoder's own PRN after the decode, which follows the slot number of string 4.
struct Receiver_Gnav_String {
    uint32_t prn;
    gnsship_gnav_string string;
};

// What the signal of the channels decides, chosen once from trk.system / trk.signal (of()).  A new signal is one more row
// of the table and the functions the row names.
struct Signal_Profile {
    enum Telemetry { NONE, GALILEO, LNAV, CNAV, DNAV, GNAV };
    using Code = std::vector<std::complex<float>>;
    char system;                      // trk.system (0: any)
    const char* signal;               // the first two characters of trk.signal (nullptr: any)
    Acq_Conf (*acq_conf)(Acq_Conf);   // the acquisition adapter's Acq_Conf (nullptr: the caller's as it stands)
    uint32_t prns;                    // set_signals_list: PRN 1..prns
    double codes_per_second;          // trk.vector_length 0 means round(fs / codes_per_second) ...
    bool own_vector_length;           // ... and L2C takes no other: one 20 ms code per epoch
    Code (*acquisition_code)(const Pcps_Acquisition_Hip& a, uint32_t prn, const Acq_Conf& acq);  // the adapter's set_local_code (empty: no such PRN)
    const char* fdma_signal;          // GLONASS: set_gnss_synchro(fdma_signal, prn) ahead of it, is_fdma()'s bias and grid
    // start_tracking's replicas: the tracked code and, where the block has a data prompt, the data code of the same length
    bool (*replicas)(uint32_t prn, bool track_pilot, std::vector<float>& tracked, std::vector<float>& data);
    Telemetry telemetry;              // the telemetry option the signal accepts ...
    int32_t telemetry_signal;         // ... and the frame type or signal of that decoder's configuration

    static const Signal_Profile& of(const Dll_Pll_Conf& trk)
    {
        static const Signal_Profile table[] = {
            // Channels_L5: acquisition on L5I, tracking on the L5Q pilot with L5I on the data prompt (start_tracking :670-678)
            {'G', "L5", gps_l5i_acq_conf, 32U, 1000.0, false,
                [](const Pcps_Acquisition_Hip&, uint32_t prn, const Acq_Conf& acq) { return gps_l5i_acquisition_code(prn, acq); }, nullptr,
                [](uint32_t prn, bool, std::vector<float>& tracked, std::vector<float>& data) {
                    tracked.resize(GPS_L5Q_CODE_LENGTH_CHIPS);
                    data.resize(GPS_L5I_CODE_LENGTH_CHIPS);
                    return gps_l5q_code_gen_float(tracked.data(), prn) && gps_l5i_code_gen_float(data.data(), prn);
                },
                CNAV, GNSSHIP_CNAV_L5},
            // Channels_2S and Channels_B3: acquisition and tracking on one code, no data prompt (start_tracking :666-668,
            // :799-801); a B3I GEO satellite is recognised by the PRN start_tracking passes on
            {'G', "2S", gps_l2_m_acq_conf, 32U, 50.0, true,
                [](const Pcps_Acquisition_Hip&, uint32_t prn, const Acq_Conf& acq) { return gps_l2c_m_acquisition_code(prn, acq); }, nullptr,
                [](uint32_t prn, bool, std::vector<float>& tracked, std::vector<float>&) {
                    tracked.resize(GPS_L2_M_CODE_LENGTH_CHIPS);
                    return gps_l2c_m_code_gen_float(tracked.data(), prn);
                },
                CNAV, GNSSHIP_CNAV_L2C},
            {'C', "B3", beidou_b3i_acq_conf, 63U, 1000.0, false,
                [](const Pcps_Acquisition_Hip&, uint32_t prn, const Acq_Conf& acq) { return beidou_b3i_acquisition_code(prn, acq); }, nullptr,
                [](uint32_t prn, bool, std::vector<float>& tracked, std::vector<float>&) {
                    tracked.resize(BEIDOU_B3I_CODE_LENGTH_CHIPS);
                    return beidou_b3i_code_gen_float(tracked.data(), static_cast<int32_t>(prn), 0);
                },
                DNAV, GNSSHIP_DNAV_B3I},
            // Channels_5X / Channels_7X: acquisition on the I component (acquire_pilot and acquire_iq at their defaults),
            // tracking on the Q pilot with the I component on the data prompt, or — trk.track_pilot false — on the I component alone
            {'E', "5X", galileo_e5_acq_conf, 36U, 1000.0, false,
                [](const Pcps_Acquisition_Hip&, uint32_t prn, const Acq_Conf& acq) { return galileo_e5_acquisition_code(prn, acq, false); }, nullptr,
                [](uint32_t prn, bool pilot, std::vector<float>& tracked, std::vector<float>& data) { return e5_replicas(false, prn, pilot, tracked, data); },
                GALILEO, GNSSHIP_TLM_FNAV},
            {'E', "7X", galileo_e5_acq_conf, 36U, 1000.0, false,
                [](const Pcps_Acquisition_Hip&, uint32_t prn, const Acq_Conf& acq) { return galileo_e5_acquisition_code(prn, acq, true); }, nullptr,
                [](uint32_t prn, bool pilot, std::vector<float>& tracked, std::vector<float>& data) { return e5_replicas(true, prn, pilot, tracked, data); },
                GALILEO, GNSSHIP_TLM_INAV},
            // Channels_1G / Channels_2G: one code for every satellite; each channel's acquisition searches under its satellite's
            // FDMA bias (pcps_acquisition::is_fdma), as the reference's channels do, and the tracker takes the frequency
            // channel from the PRN
            {'R', "1G", glonass_l1_ca_acq_conf, 24U, 1000.0, false, glonass_code, "1G", glonass_replicas, GNAV, GNSSHIP_GNAV_L1CA},
            {'R', "2G", glonass_l1_ca_acq_conf, 24U, 1000.0, false, glonass_code, "2G", glonass_replicas, GNAV, GNSSHIP_GNAV_L2CA},
            // Channels_1C, and what every other signal is run as; only system 'G' takes the LNAV decoder
            {'G', nullptr, nullptr, 32U, 1000.0, false, l1_ca_code, nullptr, l1_ca_replicas, LNAV, 0},
            {0, nullptr, nullptr, 32U, 1000.0, false, l1_ca_code, nullptr, l1_ca_replicas, NONE, 0},
        };
        const Signal_Profile* p = table;
        while ((p->system && p->system != trk.system) || (p->signal && (p->signal[0] != trk.signal[0] || p->signal[1] != trk.signal[1]))) p++;
        return *p;
    }

private:
    // start_tracking :699-746: the X primary's imaginary part tracked, its real part the data code
    static bool e5_replicas(bool band_b, uint32_t prn, bool pilot, std::vector<float>& tracked, std::vector<float>& data)
    {
        std::vector<std::complex<float>> x(GALILEO_E5A_CODE_LENGTH_CHIPS);
        const std::array<char, 3> id = {{band_b ? '7' : '5', 'X', '\0'}};
        if (!(band_b ? galileo_e5_b_code_gen_complex_primary(x.data(), static_cast<int32_t>(prn), id)
                     : galileo_e5_a_code_gen_complex_primary(x.data(), static_cast<int32_t>(prn), id)))
            return false;
        std::vector<float>& i_code = pilot ? data : tracked;
        i_code.resize(x.size());
        for (size_t i = 0; i < x.size(); i++) i_code[i] = x[i].real();
        if (pilot) tracked.resize(x.size());
        for (size_t i = 0; pilot && i < x.size(); i++) tracked[i] = x[i].imag();
        return true;
    }
    static Code glonass_code(const Pcps_Acquisition_Hip&, uint32_t, const Acq_Conf& acq) { return glonass_l1_ca_acquisition_code(acq); }
    // glonass_l1_ca_dll_pll_tracking_cc::start_tracking :198-200: the one code from chip 1
    static bool glonass_replicas(uint32_t, bool, std::vector<float>& tracked, std::vector<float>&)
    {
        std::vector<std::complex<float>> z(511);
        glonass_l1_ca_code_gen_complex(z.data(), 0);
        tracked.resize(z.size());
        for (size_t i = 0; i < z.size(); i++) tracked[i] = z[i].real();
        return true;
    }
    static Code l1_ca_code(const Pcps_Acquisition_Hip& a, uint32_t prn, const Acq_Conf& acq)
    {
        Code code(static_cast<size_t>(a.consumed_samples()));
        gnsship_gps_l1_ca_code_gen_complex_sampled(reinterpret_cast<float*>(code.data()), prn, static_cast<int32_t>(acq.fs_in), 0);
        return code;
    }
    static bool l1_ca_replicas(uint32_t prn, bool, std::vector<float>& tracked, std::vector<float>&)
    {
        tracked.resize(1023);
        gnsship_gps_l1_ca_code_gen_float(tracked.data(), static_cast<int32_t>(prn), 0);
        return true;
    }
};

class Gnss_Receiver_Hip {
public:
    explicit Gnss_Receiver_Hip(const Receiver_Conf& conf) : conf_(conf), dev_(Device::get(conf.device)), sig_(Signal_Profile::of(conf.trk))
    {
        if (sig_.acq_conf) conf_.acq = sig_.acq_conf(conf_.acq);
        n_ = std::max(1, conf_.channels);
        max_acq_ = std::min(std::max(0, conf_.in_acquisition), n_);
        conf_.satellite.resize(static_cast<size_t>(n_), 0U);
        if (conf_.trk.vector_length == 0 || sig_.own_vector_length)
            conf_.trk.vector_length = static_cast<uint32_t>(std::lround(conf_.trk.fs_in / sig_.codes_per_second));
        vl_ = static_cast<int64_t>(conf_.trk.vector_length);
        block_ = conf_.block_samples > 0 ? conf_.block_samples : static_cast<int64_t>(conf_.trk.fs_in / 10.0);
        tail_ = 2 * vl_;
        trk_ = std::make_unique<Dll_Pll_Veml_Tracking_Hip>(conf_.trk, n_, conf_.device);
        const int32_t max_ep = static_cast<int32_t>((block_ + tail_) / std::max<int64_t>(1, vl_ - 1)) + 2;  // process_block's bound
        const auto asked = [this](bool option, Signal_Profile::Telemetry kind, const char* refusal) {
            if (option && sig_.telemetry != kind) throw std::invalid_argument(refusal);
            return option;
        };
        if (asked(conf_.telemetry, Signal_Profile::GALILEO, "Gnss_Receiver_Hip: telemetry decodes Galileo channels (signal 5X or 7X)"))
            tlm_ = std::make_unique<Galileo_Telemetry_Decoder_Hip>(galileo_tlm_conf(sig_.telemetry_signal, max_ep, conf_.telemetry_mode), n_, conf_.device);
        if (asked(conf_.lnav, Signal_Profile::LNAV, "Gnss_Receiver_Hip: lnav decodes GPS L1 C/A channels (signal 1C)"))
            lnav_ = std::make_unique<Gps_L1_Ca_Telemetry_Decoder_Hip>(gps_l1_ca_tlm_conf(max_ep), n_, conf_.device);
        if (asked(conf_.cnav, Signal_Profile::CNAV, "Gnss_Receiver_Hip: cnav decodes GPS L2C or L5 channels (signal 2S or L5)"))
            cnav_ = std::make_unique<Gps_Cnav_Telemetry_Decoder_Hip>(gnsship_cnav_conf{max_ep, sig_.telemetry_signal, 0}, n_, conf_.device);
        if (asked(conf_.dnav, Signal_Profile::DNAV, "Gnss_Receiver_Hip: dnav decodes BeiDou B3I channels (signal B3)"))
            dnav_ = std::make_unique<Beidou_Dnav_Telemetry_Decoder_Hip>(gnsship_dnav_conf{max_ep, sig_.telemetry_signal, 0}, n_, conf_.device);
        if (asked(conf_.gnav, Signal_Profile::GNAV, "Gnss_Receiver_Hip: gnav decodes GLONASS channels (system R, signal 1G or 2G)"))
            gnav_ = std::make_unique<Glonass_Gnav_Telemetry_Decoder_Hip>(gnsship_gnav_conf{max_ep, sig_.telemetry_signal, 0}, n_, conf_.device);
        if (conf_.use_conditioner) {
            const double fs_out = conf_.input_filter.sampling_frequency / std::max(1, conf_.input_filter.decimation_factor);
            if (fs_out != conf_.trk.fs_in || static_cast<int64_t>(fs_out) != conf_.acq.fs_in)
                throw std::invalid_argument("Gnss_Receiver_Hip: the channels run at InputFilter.sampling_frequency / decimation_factor");
            cond_block_ = block_ * conf_.input_filter.decimation_factor;
            cond_ = std::make_unique<Freq_Xlating_Fir_Filter_Hip>(conf_.input_filter, cond_block_, conf_.device);
        }
        if (conf_.mitigation == "Pulse_Blanking_Filter")
            mit_ = std::make_unique<Pulse_Blanking_Filter_Hip>(conf_.pulse_blanking, block_, conf_.device);
        else if (conf_.mitigation == "Notch_Filter")
            mit_ = std::make_unique<Notch_Filter_Hip>(conf_.notch, block_, conf_.device);
        else if (conf_.mitigation == "Notch_Filter_Lite")
            mit_ = std::make_unique<Notch_Filter_Lite_Hip>(conf_.notch_lite, block_, conf_.device);
        else if (!conf_.mitigation.empty())
            throw std::invalid_argument("Gnss_Receiver_Hip: mitigation must be Pulse_Blanking_Filter, Notch_Filter or Notch_Filter_Lite");
        // set_signals_list (GPS: 1-32, BeiDou: 1-63, Galileo: 1-36)
        for (uint32_t p = 1; p <= sig_.prns; p++) available_.push_back(p);
        prn_.assign(static_cast<size_t>(n_), 0U);
        apos_.assign(static_cast<size_t>(n_), 0U);
        fsm_.resize(static_cast<size_t>(n_));
        for (int c = 0; c < n_; c++) {
            auto a = std::make_unique<Pcps_Acquisition_Hip>(conf_.acq, conf_.device);
            if (conf_.acq.pfa <= 0.0F) a->set_threshold(conf_.threshold);
            a->set_doppler_step(static_cast<uint32_t>(conf_.acq.doppler_step));
            if (!a->init()) throw std::runtime_error("Pcps_Acquisition_Hip::init failed");
            acq_.push_back(std::move(a));
            wire(c);
        }
        // flowgraph start: satellites assigned in channel order, the first in_acquisition channels acquire
        for (int c = 0; c < n_; c++) set_signal(c, conf_.satellite[static_cast<size_t>(c)] ? conf_.satellite[static_cast<size_t>(c)] : search_next_signal());
        state_.assign(static_cast<size_t>(n_), 0);
        for (int c = 0; c < max_acq_; c++) state_[static_cast<size_t>(c)] = 1;
        acq_count_ = max_acq_;
        for (int c = 0; c < n_; c++)
            if (state_[static_cast<size_t>(c)] == 1) start_acquisition(c);
        drain();
    }

    // Feed the next n samples of the stream (gr_complex).  Returns false on an engine error.
    bool work(const std::complex<float>* x, int64_t n)
    {
        while (n > 0) {
            const int64_t m = std::min(n, block_);
            if (!process_block(x, m)) return false;
            x += m;
            n -= m;
        }
        return true;
    }

    // With the conditioner on: feed the next n_in samples of the source in `fmt` (GNSSHIP_FMT_*; a multiple of the
    // decimation).  The stage runs on the device in pieces of one processing block; the conditioned block comes back
    // to the host, where the acquisition blocks buffer their dwells as the reference's do, and goes on to work().
    // Real (GNSSHIP_FMT_RF32 / RI16 / RI8) and bit-packed (GNSSHIP_FMT_PACKED) items too: n_in then also a multiple of
    // the samples per byte, the pieces cut at whole bytes.
    // With a mitigation filter it runs on the conditioned block while that is still on the device, and the segments it
    // completes go on to work(); without the conditioner the raw stream must be gr_complex (GNSSHIP_FMT_CF32).
    bool work_raw(const void* raw, int fmt, int64_t n_in)
    {
        if (!cond_) {
            if (!mit_ || fmt != GNSSHIP_FMT_CF32) return false;
            const std::complex<float>* x = static_cast<const std::complex<float>*>(raw);
            while (n_in > 0) {
                const int64_t m = std::min(n_in, block_);
                if (!mitigate(x, false, m)) return false;
                x += m;
                n_in -= m;
            }
            return true;
        }
        const int d = cond_->decimation();
        const int64_t bits = gnsship_cond_fmt_bits(fmt);
        if (bits == 0) return false;
        const int64_t spb = bits < 8 ? 8 / bits : 1;  // samples per byte of a packed format
        int64_t unit = d;                             // lcm(d, spb): spb is 1, 2 or 4
        while (unit % spb != 0) unit += d;
        const int64_t piece = cond_block_ - cond_block_ % unit;
        if (n_in % unit != 0 || piece == 0) return false;
        const char* p = static_cast<const char*>(raw);
        while (n_in > 0) {
            const int64_t m = std::min(n_in, piece);
            if (mit_) {
                if (!cond_->work(p, fmt, false, m)) return false;
                if (!mitigate(static_cast<const std::complex<float>*>(cond_->dev_out()), true, m / d)) return false;
            } else {
                cond_host_.resize(static_cast<size_t>(m / d));
                std::complex<float>* ho[1] = {cond_host_.data()};
                if (!cond_->work(p, fmt, false, m, nullptr, ho)) return false;
                if (!work(cond_host_.data(), m / d)) return false;
            }
            p += m * bits / 8;
            n_in -= m;
        }
        return true;
    }
    const Freq_Xlating_Fir_Filter_Hip* conditioner() const { return cond_.get(); }
    const Mitigation_Filter_Hip* mitigation() const { return mit_.get(); }

    const std::vector<Receiver_Event>& events() const { return events_; }
    // Every tracking epoch record in stream order per channel (the Gnss_Synchro stream).
    const std::vector<std::vector<Receiver_Record>>& records() const { return recs_; }
    // With conf.telemetry: every decoded page part in the order the blocks emitted them (channel by channel within a block).
    const std::vector<Receiver_Page>& pages() const { return pages_; }
    // With conf.lnav: every emitted subframe record in the order the blocks emitted them (channel by channel within a block).
    const std::vector<Receiver_Subframe>& subframes() const { return subframes_; }
    // With conf.cnav: every message record in the order the blocks emitted them (channel by channel within a block), and
    // a channel's decoder members after everything processed so far.
    const std::vector<Receiver_Cnav_Message>& cnav_messages() const { return cnav_messages_; }
    bool has_cnav() const { return cnav_ != nullptr; }
    // With conf.dnav: every subframe record in the order the blocks emitted them (channel by channel within a block).
    const std::vector<Receiver_Dnav_Subframe>& dnav_subframes() const { return dnav_subframes_; }
    // With conf.gnav: every string record in the order the blocks emitted them (channel by channel within a block), and the
    // PRN a channel's decoder is on (the assigned one until a string 4 has been decoded).
    const std::vector<Receiver_Gnav_String>& gnav_strings() const { return gnav_strings_; }
    uint32_t gnav_prn(int c) const { return gnav_ ? static_cast<uint32_t>(gnav_->state(c).prn) : 0U; }
    gnsship_cnav_state cnav_state(int c) const { return cnav_ ? cnav_->state(c) : gnsship_cnav_state{}; }
    uint64_t position() const { return pos_; }
    unsigned channel_fsm_state(int c) const { return fsm_[static_cast<size_t>(c)].state(); }
    uint32_t channel_prn(int c) const { return prn_[static_cast<size_t>(c)]; }
    int tracking_state(int c) { return trk_->state(c); }

private:
    void wire(int c)
    {
        ChannelFsm& f = fsm_[static_cast<size_t>(c)];
        f.start_acquisition = [this, c]() {  // ChannelFsm::start_acquisition → acq_->reset() (set_active)
            skip_idle(c, now_);
            acq_[static_cast<size_t>(c)]->set_active(true);
            apos_[static_cast<size_t>(c)] = now_;
            events_.push_back({now_, c, 3, prn_[static_cast<size_t>(c)], 0.0, 0.0, 0.0F});
        };
        f.stop_acquisition = [this, c]() { acq_[static_cast<size_t>(c)]->set_active(false); };
        f.start_tracking = [this, c]() {  // trk_->start_tracking(); queue (channel, 1)
            const Acq_Outcome& s = acq_[static_cast<size_t>(c)]->gnss_synchro();
            const uint32_t prn = prn_[static_cast<size_t>(c)];
            std::vector<float> tracked, data;  // the local codes as the block generates them (d_tracking_code, d_data_code)
            if (!sig_.replicas(prn, conf_.trk.track_pilot, tracked, data) ||
                !trk_->start_tracking(c, tracked.data(), data.empty() ? nullptr : data.data(), static_cast<int>(tracked.size()), s.Acq_delay_samples,
                    s.Acq_doppler_hz, s.Acq_samplestamp_samples, now_, static_cast<int>(prn)))
                error_ = true;
            queue_.push_back({c, 1});
        };
        f.stop_tracking = [this, c]() { trk_->stop_tracking(c); };
        f.request_satellite = [this, c]() { queue_.push_back({c, 0}); };
        f.notify_stop_tracking = [this, c]() { queue_.push_back({c, 2}); };
    }

    // Channel::set_signal (channel.cc:215-232): new satellite, acq_->set_local_code()
    void set_signal(int c, uint32_t prn)
    {
        prn_[static_cast<size_t>(c)] = prn;
        if (tlm_ && !tlm_->set_satellite(c)) error_ = true;  // nav_->set_satellite (channel.cc:237)
        if (lnav_ && !lnav_->new_channel(c)) error_ = true;  // the channel starts on its satellite with a new block object
        if (cnav_ && !cnav_->new_channel(c)) error_ = true;  // likewise
        if (dnav_ && !dnav_->new_channel(c, static_cast<int32_t>(prn))) error_ = true;  // likewise, constructed on the PRN
        if (gnav_ && !gnav_->new_channel(c, static_cast<int32_t>(prn))) error_ = true;  // likewise
        Pcps_Acquisition_Hip& a = *acq_[static_cast<size_t>(c)];
        const Signal_Profile::Code code = sig_.acquisition_code(a, prn, conf_.acq);
        if (code.empty() || (sig_.fdma_signal && !a.set_gnss_synchro(sig_.fdma_signal, prn)) || !a.set_local_code(code.data())) error_ = true;
    }
    void start_acquisition(int c) { fsm_[static_cast<size_t>(c)].Event_start_acquisition(); }  // Channel::start_acquisition

    // search_next_signal for GPS 1C (gnss_flowgraph.cc:2615-2629): front, rotated to the back
    uint32_t search_next_signal()
    {
        const uint32_t p = available_.front();
        available_.pop_front();
        available_.push_back(p);
        return p;
    }
    void push_back_signal(uint32_t p)
    {
        available_.remove(p);
        available_.push_back(p);
    }

    // acquisition_manager (:1797-1879)
    void acquisition_manager(int who)
    {
        for (int i = 0; i < n_; i++) {
            const int cc = (i + who + 1) % n_;
            if (acq_count_ < max_acq_ && state_[static_cast<size_t>(cc)] == 0) {
                const uint32_t sat = conf_.satellite[static_cast<size_t>(cc)];
                set_signal(cc, sat ? prn_[static_cast<size_t>(cc)] : search_next_signal());
                state_[static_cast<size_t>(cc)] = 1;
                acq_count_++;
                acq_[static_cast<size_t>(cc)]->set_doppler_center(0);  // assist_acquisition_doppler(0)
                start_acquisition(cc);
            }
        }
    }

    // apply_action (:1904-2009) for the channel events
    void apply_action(int who, int what)
    {
        const uint32_t sat = conf_.satellite[static_cast<size_t>(who)];
        const uint32_t gs = prn_[static_cast<size_t>(who)];
        if (what == 0) {
            state_[static_cast<size_t>(who)] = 0;
            if (acq_count_ > 0) acq_count_--;
            acquisition_manager(who);
            if (sat == 0) push_back_signal(gs);
        } else if (what == 1) {
            available_.remove(gs);
            state_[static_cast<size_t>(who)] = 2;
            if (acq_count_ > 0) acq_count_--;
            acquisition_manager(who);
        } else if (what == 2) {
            if (acq_count_ < max_acq_) {
                state_[static_cast<size_t>(who)] = 1;
                acq_count_++;
                set_signal(who, gs);
                start_acquisition(who);
            } else {
                state_[static_cast<size_t>(who)] = 0;
                if (sat == 0) push_back_signal(gs);
            }
        }
    }

    void drain()
    {
        while (!queue_.empty()) {
            const auto ev = queue_.front();
            queue_.erase(queue_.begin());
            apply_action(ev.first, ev.second);
        }
    }

    // an inactive acquisition block consumes the stream (general_work :912-932)
    void skip_idle(int c, uint64_t to)
    {
        Pcps_Acquisition_Hip& a = *acq_[static_cast<size_t>(c)];
        Pcps_Acquisition_Hip::Acq_Event ev;
        a.set_active(false);
        while (a.sample_counter() < to) {
            const int64_t k = std::min<int64_t>(static_cast<int64_t>(to - a.sample_counter()), 1 << 30);
            a.general_work(nullptr, static_cast<int>(k), &ev);
        }
    }

    // An acquisition decision of channel c at now_: the event, then channel_msg_receiver_cc::msg_handler_channel_events (:64-100)
    void acquisition_event(int c, Pcps_Acquisition_Hip::Acq_Event ev)
    {
        const Acq_Outcome& s = acq_[static_cast<size_t>(c)]->gnss_synchro();
        events_.push_back({now_, c, ev == Pcps_Acquisition_Hip::ACQ_SUCCESS ? 1 : 0, prn_[static_cast<size_t>(c)], s.Acq_doppler_hz, s.Acq_delay_samples,
            s.test_statistics});
        ChannelFsm& f = fsm_[static_cast<size_t>(c)];
        if (ev == Pcps_Acquisition_Hip::ACQ_SUCCESS)
            f.Event_valid_acquisition();
        else if (conf_.repeat_satellite)
            f.Event_failed_acquisition_repeat();
        else
            f.Event_failed_acquisition_no_repeat();
        drain();
    }

    // One telemetry decoder (when configured) over the records tracking left on the device: every record it emitted goes to
    // `out` with the channel's PRN (and extra(slot)...), channel by channel; a channel's fault, in the families that raise
    // them, goes back to its tracking (msg_handler_telemetry_to_trk).
    template <class Decoder, class Out, class... Extra>
    bool decode(const std::unique_ptr<Decoder>& d, std::vector<Out>& out, Extra... extra)
    {
        if (!d) return true;
        if (!d->work_trk(*trk_)) return false;
        for (int c = 0; c < n_; c++) {
            for (int k = 0; k < d->counts()[static_cast<size_t>(c)]; k++) {
                const size_t slot = static_cast<size_t>(c) * static_cast<size_t>(d->per_run()) + static_cast<size_t>(k);
                out.push_back({prn_[static_cast<size_t>(c)], d->records()[slot], extra(slot)...});
            }
            if constexpr (Decoder::has_faults)
                if (d->faults()[static_cast<size_t>(c)] && !trk_->msg_handler_telemetry_to_trk(c, 1)) return false;
        }
        return true;
    }

    bool process_block(const std::complex<float>* x, int64_t n)
    {
        const uint64_t b0 = pos_, b1 = pos_ + static_cast<uint64_t>(n);
        // 1. acquisition, in stream order over the channels acquiring
        for (;;) {
            int c = -1;
            for (int i = 0; i < n_; i++)
                if (fsm_[static_cast<size_t>(i)].state() == 1 && apos_[static_cast<size_t>(i)] < b1 &&
                    (c < 0 || apos_[static_cast<size_t>(i)] < apos_[static_cast<size_t>(c)]))
                    c = i;
            if (c < 0) break;
            Pcps_Acquisition_Hip& a = *acq_[static_cast<size_t>(c)];
            const uint64_t p = apos_[static_cast<size_t>(c)];
            const int m = static_cast<int>(std::min<uint64_t>(static_cast<uint64_t>(conf_.acq_piece), b1 - p));
            Pcps_Acquisition_Hip::Acq_Event ev = Pcps_Acquisition_Hip::ACQ_NONE;
            const int used = a.general_work(x + (p - b0), m, &ev);
            apos_[static_cast<size_t>(c)] = p + static_cast<uint64_t>(used);
            now_ = apos_[static_cast<size_t>(c)];
            if (ev != Pcps_Acquisition_Hip::ACQ_NONE) {
                acquisition_event(c, ev);
            } else if (used == 0 && !a.worker_active()) {
                // a decision is pending in state 2 (blocking: the next call makes it); a block that can
                // consume nothing more in this piece ends the channel's turn
                Pcps_Acquisition_Hip::Acq_Event ev2 = Pcps_Acquisition_Hip::ACQ_NONE;
                const int used2 = a.general_work(x + (p - b0), m, &ev2);
                apos_[static_cast<size_t>(c)] = used2 == 0 && ev2 == Pcps_Acquisition_Hip::ACQ_NONE ? b1 : p + static_cast<uint64_t>(used2);
                if (ev2 != Pcps_Acquisition_Hip::ACQ_NONE) {
                    now_ = apos_[static_cast<size_t>(c)];
                    acquisition_event(c, ev2);
                }
            }
            if (error_) return false;
        }
        // 2. tracking over [b0 − tail, b1) on the device
        const size_t keep = static_cast<size_t>(std::min<uint64_t>(static_cast<uint64_t>(tail_), b0 - win_first_));
        if (win_.size() > keep) win_.erase(win_.begin(), win_.end() - static_cast<std::ptrdiff_t>(keep));
        win_first_ = b0 - keep;
        win_.insert(win_.end(), x, x + n);
        const int64_t wn = static_cast<int64_t>(win_.size());
        if (!ensure_dev(static_cast<size_t>(wn) * sizeof(std::complex<float>))) return false;
        if (!dev_->call(gnsship_dev_upload, dev_->ctx(), dev_buf_, win_.data(), static_cast<size_t>(wn) * sizeof(std::complex<float>))) return false;
        const int max_ep = static_cast<int>(wn / std::max<int64_t>(1, vl_ - 1)) + 2;
        rec_buf_.assign(static_cast<size_t>(max_ep) * n_, gnsship_trk_epoch{});
        const bool dump = !conf_.dump_filename.empty();
        if (dump) dump_buf_.assign(static_cast<size_t>(max_ep) * n_, gnsship_trk_dump_record{});
        const int rounds = trk_->work_dump(reinterpret_cast<const std::complex<float>*>(dev_buf_), win_first_, wn, max_ep, rec_buf_.data(),
            dump ? dump_buf_.data() : nullptr, true);
        if (rounds < 0) return false;
        const auto page_bits = [this](size_t slot) {  // Galileo's one extra: the page part's data bits
            const uint8_t* b = tlm_->bits().data() + slot * static_cast<size_t>(tlm_->data_length());
            return std::vector<uint8_t>(b, b + tlm_->data_length());
        };
        if (!decode(tlm_, pages_, page_bits) || !decode(lnav_, subframes_) || !decode(cnav_, cnav_messages_) || !decode(dnav_, dnav_subframes_) ||
            !decode(gnav_, gnav_strings_))
            return false;
        recs_.resize(static_cast<size_t>(n_));
        for (int c = 0; c < n_; c++) {
            bool lost = false;
            for (int r = 0; r < rounds; r++) {
                const gnsship_trk_epoch& e = rec_buf_[static_cast<size_t>(r) * n_ + c];
                if (!(e.flags & 8)) continue;  // no epoch of this channel in this round
                recs_[static_cast<size_t>(c)].push_back({prn_[static_cast<size_t>(c)], e});
                if (e.flags & 2) lost = true;
            }
            if (dump) trk_->append_dump_file(conf_.dump_filename, c, rec_buf_.data(), dump_buf_.data(), rounds);
            if (lost) {
                now_ = b1;  // the control thread reacts after the block
                events_.push_back({now_, c, 2, prn_[static_cast<size_t>(c)], 0.0, 0.0, 0.0F});
                fsm_[static_cast<size_t>(c)].Event_failed_tracking_standby();
                drain();
            }
        }
        pos_ = b1;
        now_ = b1;
        return !error_;
    }

    bool ensure_dev(size_t bytes)
    {
        if (bytes <= dev_cap_) return true;
        std::lock_guard<std::mutex> lk(dev_->mutex());
        if (dev_buf_) gnsship_dev_free(dev_->ctx(), dev_buf_);
        dev_buf_ = nullptr;
        dev_cap_ = 0;
        if (gnsship_dev_alloc(dev_->ctx(), bytes, &dev_buf_) != GNSSHIP_OK) return false;
        dev_cap_ = bytes;
        return true;
    }

public:
    ~Gnss_Receiver_Hip()
    {
        if (dev_buf_) gnsship_dev_free(dev_->ctx(), dev_buf_);
    }

private:
    Receiver_Conf conf_;
    std::shared_ptr<Device> dev_;
    const Signal_Profile& sig_;  // what the channels' signal decides
    int n_ = 1, max_acq_ = 1, acq_count_ = 0;
    int64_t vl_ = 0, block_ = 0, tail_ = 0;
    std::unique_ptr<Dll_Pll_Veml_Tracking_Hip> trk_;
    std::unique_ptr<Galileo_Telemetry_Decoder_Hip> tlm_;  // the optional telemetry framing
    std::vector<Receiver_Page> pages_;
    std::unique_ptr<Gps_L1_Ca_Telemetry_Decoder_Hip> lnav_;  // the optional GPS L1 C/A telemetry
    std::vector<Receiver_Subframe> subframes_;
    std::unique_ptr<Gps_Cnav_Telemetry_Decoder_Hip> cnav_;  // the optional GPS CNAV telemetry (L2C or L5)
    std::vector<Receiver_Cnav_Message> cnav_messages_;
    std::unique_ptr<Beidou_Dnav_Telemetry_Decoder_Hip> dnav_;  // the optional BeiDou D1/D2 telemetry (B3I)
    std::vector<Receiver_Dnav_Subframe> dnav_subframes_;
    std::unique_ptr<Glonass_Gnav_Telemetry_Decoder_Hip> gnav_;  // the optional GLONASS GNAV telemetry (L1 or L2 C/A)
    std::vector<Receiver_Gnav_String> gnav_strings_;
    std::unique_ptr<Freq_Xlating_Fir_Filter_Hip> cond_;  // the optional conditioner stage
    int64_t cond_block_ = 0;                             // its run size, in input samples
    std::vector<std::complex<float>> cond_host_;
    std::unique_ptr<Mitigation_Filter_Hip> mit_;         // the optional interference mitigation
    // m <= block_ samples through the mitigation filter; what it emits goes to the channels
    bool mitigate(const std::complex<float>* x, bool on_device, int64_t m)
    {
        cond_host_.resize(static_cast<size_t>(block_ + GNSSHIP_MIT_MAX_LENGTH + 1));
        if (!mit_->work(x, on_device, m, nullptr, cond_host_.data())) return false;
        return mit_->n_out() == 0 || work(cond_host_.data(), mit_->n_out());
    }
    std::vector<std::unique_ptr<Pcps_Acquisition_Hip>> acq_;
    std::vector<ChannelFsm> fsm_;
    std::vector<uint32_t> prn_;
    std::vector<uint64_t> apos_;
    std::vector<int> state_;  // the flowgraph's channels_state_
    std::list<uint32_t> available_;
    std::vector<std::pair<int, int>> queue_;
    std::vector<Receiver_Event> events_;
    std::vector<std::vector<Receiver_Record>> recs_;
    std::vector<std::complex<float>> win_;
    uint64_t win_first_ = 0, pos_ = 0, now_ = 0;
    void* dev_buf_ = nullptr;
    size_t dev_cap_ = 0;
    std::vector<gnsship_trk_epoch> rec_buf_;
    std::vector<gnsship_trk_dump_record> dump_buf_;
    bool error_ = false;
};

}  // namespace gnsship

#endif  // GNSSHIP_RECEIVER_HPP
